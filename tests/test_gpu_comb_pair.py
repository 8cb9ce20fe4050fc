"""The comb ladder's column on the device (jacobian29.h: coz29_pair_sum, jpt29_rescale; verify_fast.h: the COMB block of
k_verify_fast): a round's two table entries added to each other first, their sum to the accumulator.

  (a) S2K_HP_JADD_PAIR (ops.hip: k_pair_op, the block's four lines) at exactly the lazy budgets of the interval model
      (test_comb_pair_model.py), on secp256k1 points with near-maximal limbs, once and chained 18 times with a doubling
      behind every column - the ladder's own sequence - against big-integer arithmetic; the exceptional inputs give flag = 0;
  (b) one ECDSA call of 512 signatures over 16 keys (two blocks) on per-key tables: valid signatures whose u2 = k (1 + lambda)
      and k (1 - lambda), so that a column pairs an entry with itself in both relative signs, mixed with random ones, a seeded
      tenth damaged - the oracle's verdicts byte for byte on comb and on window tables;
  (c) 512 BIP-340 signatures over 16 keys the same way (k_verify_fast<MODE_SCHNORR_COMB>)."""
import random

import numpy as np
import pytest

import pyref as R
import test_comb_pair_model as pm
import test_gpu_comb as gc
import test_gpu_schnorr_comb as sc
from test_gpu_fe29_formulas import ALL_ONES, b32, ints, lazy, secp_points

pytestmark = pytest.mark.gpu
P, N = R.P, R.N
NSIG, NKEYS = 512, 16


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _phi(pt):
    return (pt[0] * R.BETA % P, pt[1])


def _signed(pt, neg):
    return R.neg(pt) if neg and pt is not None else pt


def _col(vals):
    return [b32(v) for v in vals]


def _operands(rnd, count):
    """P, E1, E2' = phi(E2) (its x is what the ladder passes: beta * x) and the sign bits of `count` lanes"""
    pts = secp_points(rnd, count)
    ps, e1, e2 = pts, pts[3:] + pts[:3], [_phi(q) for q in pts[7:] + pts[:7]]
    sg = [i & 3 for i in range(count)]
    return ps, e1, e2, sg


def _chain_ref(p, a, b, s, reps):
    """reps == 0: P + T for T = s1 E1 + s2 E2'; else `reps` times acc = 2 (acc + T), as k_pair_op chains the column"""
    t = R.add(_signed(a, s & 1), _signed(b, s & 2))
    if reps == 0:
        return R.add(p, t)
    for _ in range(reps):
        p = R.add(p, t)
        p = R.add(p, p)
    return p


def _run(eng, ps, e1, e2, sg, codes, reps, z=None):
    import secp256k1_voi_amd as S
    px, py, x1, y1, x2, y2 = codes
    cols = [_col(p[0] for p in ps), _col(p[1] for p in ps), None if z is None else _col(z), _col(q[0] for q in e1), _col(q[1] for q in e1),
            _col(q[0] for q in e2), _col(q[1] for q in e2), _col(sg)]
    x, y, flag = eng.fp_op_batch_ex8(S.HP_JADD_PAIR, cols, lazy(px, py, 8 if z is None else 0, x1, y1, x2, y2, 0), reps)
    return list(zip(ints(x), ints(y))), list(flag)


@pytest.mark.parametrize("codes", pm.pair_budgets() + [(0,) * 6])
@pytest.mark.parametrize("reps", [0, 18])
def test_column_at_model_budget(eng, codes, reps):
    """P = (a, b, 1) and the entries in their lazy forms at the model's largest codes; all four sign pairs"""
    rnd = random.Random(1830 + sum(codes) + reps)
    ps, e1, e2, sg = _operands(rnd, 64)
    got, flag = _run(eng, ps, e1, e2, sg, codes, reps)
    for p, a, b, s, g, f in zip(ps, e1, e2, sg, got, flag):
        assert a[0] != b[0] and f == 1 and g == _chain_ref(p, a, b, s, reps), (p, a, b, s, reps)


def test_column_over_a_common_z(eng):
    """the table's points over a common Z = w (on the curve isomorphic by w) and the accumulator with a Z of its own"""
    rnd = random.Random(1840)
    ps, e1, e2, sg = _operands(rnd, 64)
    ws = [rnd.randrange(2, P) for _ in ps]
    ws[:3] = [P - 1, ALL_ONES, 2]
    za = [rnd.randrange(1, P) for _ in ps]
    za[:4] = [1, P - 1, ALL_ONES, 2]
    iso = lambda pts: [(q[0] * w * w % P, q[1] * pow(w, 3, P) % P) for q, w in zip(pts, ws)]
    for reps in (0, 18):
        got, flag = _run(eng, iso(ps), iso(e1), iso(e2), sg, (0,) * 6, reps, z=za)
        for p, a, b, s, w, g, f in zip(ps, e1, e2, sg, ws, got, flag):
            e = _chain_ref(p, a, b, s, reps)
            assert f == 1 and g == (e[0] * w * w % P, e[1] * pow(w, 3, P) % P), (p, a, b, s, reps)


def test_exceptional_inputs_give_flag_zero(eng):
    """E1 = E2' and E1 = -E2' (h = 0), acc = +-T, acc.z = 0: Z3 = 0, once and through a chain (Z = 0 is sticky)"""
    rnd = random.Random(1850)
    ps, e1, e2, sg = _operands(rnd, 48)
    kinds = [i % 6 for i in range(len(ps))]
    z = [rnd.randrange(1, P) for _ in ps]
    for i, k in enumerate(kinds):
        s = sg[i]
        if k == 0:                                     # E1 = E2'
            e2[i] = e1[i]
        elif k == 1:                                   # E1 = -E2'
            e2[i] = R.neg(e1[i])
        elif k in (2, 3):                              # acc = T, acc = -T
            t = R.add(_signed(e1[i], s & 1), _signed(e2[i], s & 2))
            ps[i] = t if k == 2 else R.neg(t)
        elif k == 4:                                   # acc.z = 0
            z[i] = 0
    for reps in (0, 18):
        got, flag = _run(eng, ps, e1, e2, sg, (0,) * 6, reps, z=z)
        for i, k in enumerate(kinds):
            if k < 5:
                assert flag[i] == 0, (i, k, reps)
            elif reps == 0:
                assert flag[i] == 1 and got[i] == _chain_ref(ps[i], e1[i], e2[i], sg[i], 0), i


# ==== whole calls ==========================================================================================================
def _rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), np.uint8).reshape(-1, 32).copy()


@pytest.fixture(scope="module")
def ecdsa_batch(eng):
    """512 valid signatures of 16 keys: R = (u1 + u2 d) G, r = x(R) mod n, s = r / u2, e = u1 s (test_gpu_comb.py's construction);
    the first half with the paired u2, the second with random ones, shuffled"""
    rng = random.Random(1861)
    d = [rng.randrange(1, N) for _ in range(NKEYS)]
    u2 = pm.paired_u2(rng, NSIG // 2) + [rng.randrange(1, N) for _ in range(NSIG // 2)]
    rng.shuffle(u2)
    key = [i % NKEYS for i in range(NSIG)]
    u1 = [rng.randrange(1, N) for _ in range(NSIG)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    assert all(kR)
    Rp = eng.scalar_base_mult_batch(_rows(kR))
    Q = eng.scalar_base_mult_batch(_rows(d))[:, 1:]
    rr = [int.from_bytes(bytes(Rp[i, 1:33]), "big") % N for i in range(NSIG)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    assert all(rr) and all(ss)
    return np.ascontiguousarray(Q[key]), _rows(ee), _rows(rr), _rows(ss)


def test_ecdsa_call_with_paired_columns(eng, oracle, ecdsa_batch):
    pub, dig, r, s = (a.copy() for a in ecdsa_batch)
    exp, st = gc._both_ladders(eng, oracle, pub, dig, r, s)          # (checks last_keyed_ladder() for both ladders)
    assert exp.all() and st["keyed"] == NSIG and st["tables"] == NKEYS
    assert st["complete"] == 0, "an undamaged signature reached the complete-formula worklist"
    g = np.random.default_rng(1862)
    hit = g.permutation(NSIG)[:NSIG // 10]
    for arr, part in zip((r, s, dig), np.array_split(hit, 3)):
        arr[part, g.integers(0, 32, size=part.size)] ^= (1 << g.integers(0, 8, size=part.size)).astype(np.uint8)
    exp, st = gc._both_ladders(eng, oracle, pub, dig, r, s)
    assert st["keyed"] == NSIG and not exp[hit].any() and exp.sum() == NSIG - len(hit)


def test_schnorr_call(eng, oracle):
    """512 BIP-340 signatures of 16 keys, a seeded tenth damaged, on comb and on window tables (mode 17 and mode 6)"""
    rng = random.Random(1870)
    d = [rng.randrange(1, N) for _ in range(NKEYS)]
    key = [i % NKEYS for i in range(NSIG)]
    msgs = [rng.randbytes(sc.MSG_LENGTHS[i % len(sc.MSG_LENGTHS)]) for i in range(NSIG)]
    pk, sig, _ = sc.sign(eng, d, key, msgs, rng)
    hit = np.random.default_rng(1871).permutation(NSIG)[:NSIG // 10].tolist()
    for j, i in enumerate(hit):
        s_ = bytearray(sig[i])
        s_[32 * (j & 1) + rng.randrange(32)] ^= 1 << rng.randrange(8)
        sig[i] = bytes(s_)
    exp = sc.expected(oracle, pk, msgs, sig)
    assert not exp[hit].any() and exp.sum() == NSIG - len(hit)
    st = sc.both_ladders(eng, pk, msgs, sig, exp)
    assert st["keyed"] == NSIG and st["tables"] == NKEYS
