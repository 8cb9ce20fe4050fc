"""Arithmetic mod n on the device, operation by operation, against Python integers - and the shared inversion of the
scalar preparation end to end.

* sc26.h (the lazy 10 x 26 Montgomery form, R = 2^260, of k_scalar_prep / scalar_prep_one: u1 = e/s, u2 = r/s) through
  s2k_fp_op_batch_ex's HP_SC26_* codes, with operands in [n, 2n) on purpose (the lazy code adds n; [2^256, 2n) included),
  its raw results checked against the lazy contract (< 2n, limbs in bounds) as well as for their value;
* sc.h (8 x 32, canonical: the BIP-340 whole-batch coefficients a_i e_i, the FORCE_COMPLETE and recovery fallback
  kernels) through the HP_SC_* codes;
* Montgomery's trick over PREP_M items per lane: invalid s (ECDSA) or r (recovery) is replaced by 1 in the lane's
  product; the damaged items and every lane-mate of one must still get the oracle's answer, at sizes where lanes share an
  inversion (n > 2^16), a ragged last lane included.

The CPU model of the generated 10 x 26 product is tests/test_sc26_model.py.
"""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
R26, R32 = 1 << 260, 1 << 256
HALF_N = (N - 1) // 2
M26 = (1 << 26) - 1
PREP_M = 6
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    assert "PREP_M=%d" % PREP_M in S.load_library().s2k_build_config().decode()
    return e


def rows(vals):
    return np.frombuffer(b"".join((v % R32).to_bytes(32, "big") for v in vals), np.uint8).reshape(-1, 32).copy()


def ints(arr):
    return [int.from_bytes(bytes(r), "big") for r in arr]


def limbs_value(ls):
    return sum(x << (26 * i) for i, x in enumerate(ls))


# ---- operand pools ---------------------------------------------------------------------------------------------------
EDGES = [0, 1, 2, N - 1, N, N + 1, (N - 1) // 2, (N + 1) // 2, 2**128 - 1, 2**128, 2**128 + 1, 2**255, 2**256 - 1,
         LAMBDA, N - LAMBDA, R26 % N, R32 % N, pow(R26, -1, N), pow(R32, -1, N)]


def structured_26(rng):
    """limb patterns of the 10 x 26 form (limb 9 < 2^22: the value fits the 32-byte operand)"""
    nl = [(N >> (26 * i)) & M26 for i in range(10)]
    out = []
    for fill in (0, 1, M26, 1 << 25):
        for top in (0, 1, (1 << 22) - 1, nl[9]):
            out.append(limbs_value([fill] * 9 + [top]))
    for k in range(10):
        for d in (-1, 1):
            v = list(nl)
            v[k] = (v[k] + d) & (M26 if k < 9 else (1 << 22) - 1)
            out.append(limbs_value(v))
    for _ in range(64):
        out.append(limbs_value([rng.choice((0, 1, M26, 1 << 25, nl[i])) for i in range(9)] + [rng.choice((0, (1 << 22) - 1, nl[9]))]))
    return out


def structured_32(rng):
    """word patterns of the 8 x 32 form, canonical"""
    nw = [(N >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    out = []
    for fill in (0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF):
        for k in range(8):
            out.append(sum((fill if j <= k else 0) << (32 * j) for j in range(8)))
    for k in range(8):
        for d in (-1, 1):
            v = list(nw)
            v[k] = (v[k] + d) & 0xFFFFFFFF
            out.append(sum(x << (32 * j) for j, x in enumerate(v)))
    for _ in range(64):
        out.append(sum(rng.choice((0, 1, 0xFFFFFFFF, 0x80000000, nw[j])) << (32 * j) for j in range(8)))
    return [v for v in out if v < N]


def pool(rng, count, canonical):
    p = EDGES + structured_26(rng) + structured_32(rng) + [rng.randrange(N) for _ in range(count)]
    if not canonical:
        p += [rng.randrange(N, R32) for _ in range(count // 8)]
    p = [v for v in p if v < (N if canonical else R32)]
    rng.shuffle(p)
    return p


def pairs(rng, count, canonical):
    a = pool(rng, count, canonical)
    b = pool(rng, count, canonical)[:len(a)]
    a = a[:len(b)]
    return a + EDGES * len(EDGES), b + [y for y in EDGES for _ in EDGES]        # + every pair of edge values


# ---- sc26.h ----------------------------------------------------------------------------------------------------------
def sc26_call(eng, op, a, b, codes, reps=0):
    import secp256k1_voi_amd as S
    lazy = codes[0] | (codes[1] << 4) | (reps << 20)
    ops = [rows(a)] + ([rows(b)] if b is not None else [])
    out, out2, flag = eng.fp_op_batch_ex(getattr(S, op), ops, lazy)
    raw = [v + ((int(f) & 1) << 256) for v, f in zip(ints(out), flag)]
    return raw, ints(out2), flag


def check_sc26(raw, canon, flag, expect, what):
    for i, (r, c, f, e) in enumerate(zip(raw, canon, flag, expect)):
        assert f & 2, (what, i, "limbs out of bounds")
        assert r < 2 * N, (what, i, "raw result >= 2n", hex(r))
        assert r % N == e % N and c == e % N, (what, i, hex(r), hex(e % N))


CODES = [(0, 0), (1, 0), (0, 1), (1, 1)]       # canonical x canonical, lazy x canonical, canonical x lazy, lazy x lazy


def lazy_value(v, code):
    return v + N * (code & 1)


@pytest.mark.parametrize("codes", CODES)
def test_sc26_mul_sqr_on_lazy_operands(eng, codes):
    # the products take any limbs within the bounds (the model in test_sc26_model.py), so the lazy code is also applied to
    # inputs in [n, 2^256): up to 2^256 + n, beyond 2n, and the result must still be < 2n
    rng = random.Random(0x260 + codes[0] * 2 + codes[1])
    a, b = pairs(rng, 3000, canonical=codes != (0, 0))
    R_INV = pow(R26, -1, N)
    la, lb = [lazy_value(x, codes[0]) for x in a], [lazy_value(x, codes[1]) for x in b]
    raw, canon, flag = sc26_call(eng, "HP_SC26_MUL", a, b, codes)
    check_sc26(raw, canon, flag, [x * y * R_INV for x, y in zip(la, lb)], "SC26_MUL")
    raw2, _, _ = sc26_call(eng, "HP_SC26_MUL", b, a, codes[::-1])
    assert raw2 == raw                                           # both factor orders: same limbs
    raw, canon, flag = sc26_call(eng, "HP_SC26_SQR", a, None, codes)
    check_sc26(raw, canon, flag, [x * x * R_INV for x in la], "SC26_SQR")
    # the square is the product of a value with itself, limb for limb
    raw2, _, _ = sc26_call(eng, "HP_SC26_MUL", a, a, (codes[0], codes[0]))
    assert raw2 == raw


@pytest.mark.parametrize("code", [0, 1])
def test_sc26_conversions_and_inverse(eng, code):
    # sc26_to_sc (and the inversion, which starts with it) takes lazy values, < 2n: with the lazy code on, canonical inputs
    rng = random.Random(0x26C + code)
    a = pool(rng, 2000, canonical=code == 1)
    la = [lazy_value(x, code) for x in a]
    assert all(x < 2 * N for x in la)
    raw, canon, flag = sc26_call(eng, "HP_SC26_TO_MONT", a, None, (code, 0))
    check_sc26(raw, canon, flag, [x * R26 for x in la], "SC26_TO_MONT")
    raw, canon, flag = sc26_call(eng, "HP_SC26_TO_SC", a, None, (code, 0))
    assert raw == la and canon == [x % N for x in la]           # the lazy input went in as it should, and is reduced
    assert all(f & 2 for f in flag)
    # [2^256, 2n) reached: the inputs sc26_to_sc must take bit 256 of
    assert code == 0 or any(x >= R32 for x in la)
    sub = a[:600] + [0, N - 1, 1] + ([N] if code == 0 else [])      # 0 -> 0, n (= 0) too
    raw, canon, flag = sc26_call(eng, "HP_SC26_INV", sub, None, (code, 0))
    lsub = [lazy_value(x, code) for x in sub]
    check_sc26(raw, canon, flag, [0 if x % N == 0 else pow(x, -1, N) * R26 * R26 for x in lsub], "SC26_INV")


def test_sc26_products_that_land_in_n_to_2p256(eng):
    # A raw product below 2^256 but not below n: random operands land there with probability ~2^-128, so these are
    # constructed - a * b = v R (mod n) with a b < v R makes the reduction's quotient m = (v R - a b) / n < R and the raw
    # result exactly v.  sc26_to_sc (u1 = e/s, u2 = r/s of k_scalar_prep) must still subtract n.
    rng = random.Random(0x2256)
    vs = [N + d for d in [1, 2, 2**64, 2**100, R32 - N - 1, R32 - N - 2] + [rng.randrange(1, R32 - N) for _ in range(250)]]
    a = [rng.choice((2**200 + 12345, rng.randrange(2**250, N))) for _ in vs]
    b = [v * R26 * pow(x, -1, N) % N for v, x in zip(vs, a)]
    raw, canon, flag = sc26_call(eng, "HP_SC26_MUL", a, b, (0, 0))
    assert raw == vs
    check_sc26(raw, canon, flag, vs, "SC26_MUL into [n, 2^256)")


@pytest.mark.parametrize("reps", [1, PREP_M, 64])
def test_sc26_chain(eng, reps):
    rng = random.Random(reps)
    for codes in CODES:
        a, b = pairs(rng, 1000, canonical=False)
        la, lb = [lazy_value(x, codes[0]) for x in a], [lazy_value(x, codes[1]) for x in b]
        raw, canon, flag = sc26_call(eng, "HP_SC26_CHAIN", a, b, codes, reps)
        f = pow(pow(R26, -1, N), reps, N)
        check_sc26(raw, canon, flag, [x * pow(y, reps, N) * f for x, y in zip(la, lb)], ("SC26_CHAIN", reps, codes))


def test_sc26_prep_chain_shape(eng):
    # as k_scalar_prep: acc = R, acc = acc * to_mont(s_i); s_i^-1 R = inv * prefix_{i-1}; inv = inv * s_i R
    rng = random.Random(66)
    s = [rng.randrange(1, N) for _ in range(2048)] + [1, N - 1, 2, (N + 1) // 2]
    raw, canon, flag = sc26_call(eng, "HP_SC26_TO_MONT", s, None, (0, 0))
    sm = raw
    one_m = [R26 % N] * len(s)
    # sm values may lie in [n, 2n): feed them back raw through the lazy code where they are canonical + n
    lazy_in = [(v - N, 1) if v >= N else (v, 0) for v in sm]
    for code in (0, 1):
        sel = [i for i, (_, c) in enumerate(lazy_in) if c == code]
        if not sel:
            continue
        raw, canon, flag = sc26_call(eng, "HP_SC26_MUL", [one_m[i] for i in sel], [lazy_in[i][0] for i in sel], (0, code))
        check_sc26(raw, canon, flag, [s[i] * R26 for i in sel], "prep first product")


# ---- sc.h ------------------------------------------------------------------------------------------------------------
def sc_call(eng, op, a, b=None):
    import secp256k1_voi_amd as S
    ops = [rows(a)] + ([rows(b)] if b is not None else [])
    out, _, flag = eng.fp_op_batch_ex(getattr(S, op), ops, 0)
    return ints(out), flag


def test_sc_ops_canonical(eng):
    rng = random.Random(0x832)
    a, b = pairs(rng, 3000, canonical=True)
    keep = [i for i in range(len(a)) if a[i] < N and b[i] < N]
    a, b = [a[i] for i in keep], [b[i] for i in keep]
    R_INV = pow(R32, -1, N)
    out, _ = sc_call(eng, "HP_SC_MONTMUL", a, b)
    assert out == [x * y * R_INV % N for x, y in zip(a, b)]
    out, _ = sc_call(eng, "HP_SC_TO_MONT", a)
    assert out == [x * R32 % N for x in a]
    out, _ = sc_call(eng, "HP_SC_ADD", a, b)
    assert out == [(x + y) % N for x, y in zip(a, b)]
    out, _ = sc_call(eng, "HP_SC_NEG", a)
    assert out == [(-x) % N for x in a]
    out, flag = sc_call(eng, "HP_SC_GT_HALF_N", a)
    assert list(flag) == [int(x > HALF_N) for x in a]
    half = [HALF_N - 1, HALF_N, HALF_N + 1, N - 1, 0]
    _, flag = sc_call(eng, "HP_SC_GT_HALF_N", half)
    assert list(flag) == [0, 0, 1, 1, 0]
    sub = a[:400] + [0, 1, N - 1, 2]
    out, _ = sc_call(eng, "HP_SC_MONT_INV", sub)                 # the Fermat chain: x R -> x^-1 R
    assert out == [0 if x == 0 else pow(x, -1, N) * R32 * R32 % N for x in sub]


def test_sc_reduce_once_and_raw_first_factor(eng):
    rng = random.Random(0x833)
    raw = pool(rng, 2000, canonical=False) + [N, N + 1, R32 - 1, 2 * N - R32, R32 - N]
    out, _ = sc_call(eng, "HP_SC_REDUCE_ONCE", raw)
    assert out == [x % N for x in raw]
    # a < 2^256 times a canonical b stays below 2n before the final subtraction: exact for raw first factors too
    b = [rng.randrange(N) for _ in raw]
    out, _ = sc_call(eng, "HP_SC_MONTMUL", raw, b)
    assert out == [x * y * pow(R32, -1, N) % N for x, y in zip(raw, b)]


def test_rlc_coefficient_shape(eng):
    # k_schnorr_rlc_prep: a_m = to_mont(a), a < 2^128; a e = montmul(e, a_m), a s = montmul(s, a_m)
    rng = random.Random(0x4C)
    a = [1, 2**128 - 1, 2**127, 3] + [rng.randrange(2**128) for _ in range(3000)]
    e = [N - 1, N - 1, 0, HALF_N] + [rng.choice((rng.randrange(N), N - 1 - rng.randrange(2**32))) for _ in range(3000)]
    am, _ = sc_call(eng, "HP_SC_TO_MONT", a)
    out, _ = sc_call(eng, "HP_SC_MONTMUL", e, am)
    assert out == [x * y % N for x, y in zip(a, e)]


# ---- the shared inversion end to end ---------------------------------------------------------------------------------
DAMAGE = [0, N, N + 1, R32 - 1]


def prep_lanes(n):
    return max((n + PREP_M - 1) // PREP_M, min(n, 1 << 16))


def lane_items(t, T, n):
    return [t + j * T for j in range(PREP_M) if t + j * T < n]


def damage_plan(n, rng, n_single=300, n_lanes=40):
    """(single, whole): single damaged items whose lane-mates stay valid, and whole lanes damaged; lanes as
    k_scalar_prep deals them for a call of n (T = prep_lanes(n)) and for the first piece of a pinned call"""
    T = prep_lanes(n)
    taken = set()
    whole = []
    lanes = [0, T - 1, (n - 1) % T] + [rng.randrange(T) for _ in range(n_lanes)]
    per = ((n + 3) // 4 + 255) & ~255 if n >= (1 << 16) else n     # the pieces of a pinned call
    Tc = prep_lanes(min(per, n))
    for t in lanes[:n_lanes // 2]:
        for i in lane_items(t, T, n):
            if i not in taken:
                taken.add(i)
                whole.append(i)
    for t in lanes[n_lanes // 2:]:
        for i in lane_items(t % Tc, Tc, min(per, n)):
            if i not in taken:
                taken.add(i)
                whole.append(i)
    single = []
    while len(single) < n_single:
        i = rng.randrange(n)
        mates = set(lane_items(i % T, T, n))
        if mates & taken:
            continue
        taken.add(i)
        single.append(i)
    single += [n - 1] if n - 1 not in taken else []
    return single, whole, T


def put(arr, idx, vals):
    for i, v in zip(idx, vals):
        arr[i] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)


@pytest.mark.parametrize("n", [(1 << 16) + 1, 6 * (1 << 16) + 5, (1 << 20) - 3])
def test_ecdsa_shared_inversion_with_invalid_s(eng, oracle, n):
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = synth_batch(eng, n, 1 << 12, seed=0x5C00 + (n & 0xFF))
    rng = random.Random(n)
    single, whole, T = damage_plan(n, rng)
    damaged = single + whole
    put(s, damaged, [DAMAGE[k % 4] for k in range(len(damaged))])
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=THREADS)
    assert not exp[damaged].any()
    valid = np.ones(n, bool)
    valid[damaged] = False
    assert exp[valid].all()
    got = eng.ecdsa_verify_batch(pub, dig, r, s)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    pinned = [S.pinned_array(a.shape) for a in (pub, dig, r, s)]
    for d, a in zip(pinned, (pub, dig, r, s)):
        d[...] = a
    got = eng.ecdsa_verify_batch(*pinned)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    if n < (1 << 17):
        got = eng.ecdsa_verify_batch(pub, dig, r, s, force_complete=True)
        assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]


@pytest.mark.parametrize("n", [(1 << 16) + 1, 6 * (1 << 16) + 5, (1 << 20) - 3])
def test_recovery_shared_inversion_with_invalid_r(eng, oracle, n):
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = synth_batch(eng, n, 1 << 12, seed=0x4E00 + (n & 0xFF))
    rid = np.zeros(n, dtype=np.uint8)
    rec, ok = eng.ecdsa_recover_batch(dig, r, s, rid)
    rid[(rec[:, 1:] != pub).any(axis=1)] = 1                          # the right id of every valid signature
    rng = random.Random(n + 1)
    single, whole, T = damage_plan(n, rng, n_single=150, n_lanes=20)
    damaged = single + whole
    put(r, damaged, [DAMAGE[k % 4] for k in range(len(damaged))])
    mates = sorted({m for i in single for m in lane_items(i % T, T, n)} - set(damaged))
    runs = [False, True] if n < (1 << 17) else [False]
    for fc in runs:
        rec, ok = eng.ecdsa_recover_batch(dig, r, s, rid, force_complete=fc)
        for j in damaged + mates:
            e = oracle.ecdsa_recover(bytes(dig[j]), bytes(r[j]), bytes(s[j]), int(rid[j]))
            assert (bytes(rec[j]) == e and ok[j] == 1) if e is not None else (ok[j] == 0 and not rec[j].any()), (fc, j)
        assert not ok[damaged].any()
        untouched = np.ones(n, bool)
        untouched[damaged] = False
        assert ok[untouched].all() and (rec[untouched][:, 1:] == pub[untouched]).all() and (rec[untouched][:, 0] == 4).all()
