"""Small calls over a COMB key set: the wave-per-signature ladder on the set's comb tables (small_call.hip: row_ladder_comb,
k_verify_row_comb, k_schnorr_row_comb; fe29r.h: pt29r_pair_from_iso - an entry (x, y) of y^2 = x^3 + 7 W^6 is (x W : y : W^3) on
secp256k1), opt-in through set_keyset_comb_small_batch_max.

Every verdict is compared with the CPU oracle's on the expanded keys (the oracle's schnorr_verify for BIP-340) and with the
same call on the lane-per-signature path (the knob at 0, what a new engine has); last_keyset_ladder() says which of the two
ran.  A round of the ladder runs through the C-ABI (S2K_HP_PT29R_COMB_STEP) against the affine group law.  Every case is a
well-formed call whose verdict is data."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_comb as TC
import test_gpu_keyset_row as KR
import test_gpu_schnorr_comb as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
N, P = R.N, R.P
b32 = R.b32
SIZES = KR.SIZES                      # 1, 3, 4, 5, 255, 1024: a lone wave, a partial block, a whole block, a block and a wave, many blocks
KNOB = 3072
ZERO_STATS = {"keyed": 0, "tables": 0, "general": 0, "complete": 0}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _row_and_lane(eng, call, exp):
    """call() with the knob at 3072 and at 0: both give `exp`; ROW_COMB with zero grouping statistics, then LANE"""
    import secp256k1_voi_amd as S
    try:
        eng.set_keyset_comb_small_batch_max(KNOB)
        got = call()
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_ROW_COMB
        assert eng.key_grouping_stats() == ZERO_STATS
        eng.set_keyset_comb_small_batch_max(0)
        lane = call()
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
    finally:
        eng.set_keyset_comb_small_batch_max(0)
    assert np.array_equal(got, exp), np.nonzero(np.asarray(got) != np.asarray(exp))[0][:10]
    assert np.array_equal(lane, exp), np.nonzero(np.asarray(lane) != np.asarray(exp))[0][:10]
    return got


def test_new_symbols_default_and_threshold():
    """A fresh engine sends a comb set's small call to the lane path; with the knob at max_n a call of max_n signatures takes
    the row ladder and one of max_n + 1 does not; S2K_ECDSA_FORCE_WORKLIST keeps the lane path; the threshold of the other
    layouts does not govern comb sets."""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    assert (S.KEYSET_LADDER_LANE, S.KEYSET_LADDER_ROW, S.KEYSET_LADDER_ROW_COMB) == (0, 1, 2)
    assert S.HP_PT29R_COMB_STEP == S.HP_JADD_PAIR + 1
    e2 = S.Engine(0)
    try:
        max_n = 300
        pub, dig, r, s = (np.array(a) for a in synth_batch(e2, max_n + 1, 1, seed=2110))
        zeros = np.zeros(max_n + 1, np.uint32)
        ks = e2.keyset_create(pub[:1], S.KEYSET_COMB)
        try:
            assert e2.last_keyset_ladder() == -1
            assert e2.ecdsa_verify_batch_keyset(ks, zeros[:8], dig[:8], r[:8], s[:8]).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_LANE
            e2.set_keyset_small_batch_max(1 << 20)
            assert e2.ecdsa_verify_batch_keyset(ks, zeros[:8], dig[:8], r[:8], s[:8]).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_LANE
            e2.set_keyset_comb_small_batch_max(max_n)
            assert e2.ecdsa_verify_batch_keyset(ks, zeros[:-1], dig[:-1], r[:-1], s[:-1]).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_ROW_COMB
            assert e2.key_grouping_stats() == ZERO_STATS
            assert e2.ecdsa_verify_batch_keyset(ks, zeros, dig, r, s).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_LANE
            got = e2.ecdsa_verify_batch_keyset(ks, zeros[:64], dig[:64], r[:64], s[:64], force_worklist=True)
            assert got.all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_LANE and e2.key_grouping_stats()["complete"] == 64
            # ... and a chunk set's small call does not read the comb sets' knob
            e2.set_keyset_small_batch_max(0)
            ck = e2.keyset_create(pub[:1], S.KEYSET_CHUNKS)
            try:
                assert e2.ecdsa_verify_batch_keyset(ck, zeros[:8], dig[:8], r[:8], s[:8]).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_LANE
            finally:
                ck.close()
        finally:
            ks.close()
    finally:
        e2.close()


@pytest.mark.parametrize("ylazy", [0, 1])
def test_pt29r_comb_step_op(eng, ylazy):
    """S2K_HP_PT29R_COMB_STEP on 64 items, 1 and 18 rounds: Q goes to y^2 = x^3 + 7 W^6 and comes back as (x W : y : W^3), the
    accumulator starts at P and each round doubles it and adds Q: 2^reps P + (2^reps - 1) Q of the affine law.  Q = P; Q = -2 P
    (the first round lands on the identity); Q = 2 P (the first addition meets equal points); the identity as P, as Q and as
    both ((0, 0) stands for it); W = 1 and W = p - 1; both lazy codes of y.  Flag 2 would mean the rows of a wave disagree."""
    import secp256k1_voi_amd as S
    rnd = random.Random(2120 + ylazy)
    n = 64
    pts = [R.mul(rnd.randrange(1, N), R.G) for _ in range(n)]
    qs = [R.mul(rnd.randrange(1, N), R.G) for _ in range(n)]
    for i in range(n):
        kind = i % 8
        if kind == 1:
            qs[i] = pts[i]
        elif kind == 2:
            qs[i] = R.neg(R.add(pts[i], pts[i]))
        elif kind == 3:
            qs[i] = R.add(pts[i], pts[i])
        elif kind == 4:
            pts[i] = None
        elif kind == 5:
            qs[i] = None
        elif kind == 6 and i % 16 == 6:
            pts[i] = qs[i] = None
    w = [rnd.randrange(1, P) for _ in range(n)]
    w[0], w[7], w[2], w[3] = 1, P - 1, 1, P - 1
    xy = lambda pt: pt if pt is not None else (0, 0)
    cols = [[b32(xy(p)[0]) for p in pts], [b32(xy(p)[1]) for p in pts], [b32(v) for v in w],
            [b32(xy(q)[0]) for q in qs], [b32(xy(q)[1]) for q in qs]]
    seen_identity = 0
    for reps in (1, 18):
        x, y, flag = eng.fp_op_batch_ex(S.HP_PT29R_COMB_STEP, cols, ylazy | reps << 20)
        assert 2 not in set(int(f) for f in flag)
        for i, (xi, yi, f) in enumerate(zip(KR._ints(x), KR._ints(y), flag)):
            e = R.add(R.mul(2 ** reps, pts[i]) if pts[i] else None, R.mul(2 ** reps - 1, qs[i]) if qs[i] else None)
            if e is None:
                assert f == 0, (i, reps, f)
                seen_identity += 1
            else:
                assert f == 1 and (xi, yi) == e, (i, reps, f)
    assert seen_identity >= 8 + 2                      # Q = -2 P at one round, and the identity on both sides at either count


@pytest.fixture(scope="module")
def ecdsa_1024(eng, oracle):
    keys, kidx, full, dig, r, s = KR._ecdsa_batch(eng, 1024, 8, 2130)
    exp = {rm: oracle.ecdsa_verify_batch(full, dig, r, s, reject_malleable=rm, nthreads=min(16, os.cpu_count() or 1)) for rm in (False, True)}
    assert 0 < exp[True].sum() < exp[False].sum() < 1024
    return keys, kidx, full, dig, r, s, exp


def test_ecdsa_row_ladder_over_a_comb_set(eng, ecdsa_1024):
    """8 keys and two set entries that are no keys, n = 1, 3, 4, 5, 255, 1024, a tenth damaged, every ninth with high s, indices
    outside the set, both reject_malleable values: the oracle's verdicts on the expanded keys, the lane path's, and ROW_COMB /
    LANE reported.  Fails on a library without the ladder (the setter is missing there)."""
    import secp256k1_voi_amd as S
    keys, kidx, full, dig, r, s, exp = ecdsa_1024
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        assert ks.layout() == S.KEYSET_COMB and ks.valid_keys().tolist() == [1] * (len(keys) - 2) + [0, 0]
        for n in SIZES:
            lo = 1024 - n if n < 255 else 0                                   # (small slices from the end, large from the start)
            sl = slice(lo, lo + n)
            for rm in (False, True):
                got = _row_and_lane(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx[sl], dig[sl], r[sl], s[sl], reject_malleable=rm), exp[rm][sl])
            if n == 1024:
                outside = kidx >= len(keys) - 2
                assert outside.sum() >= 8 and not got[outside].any()
    finally:
        ks.close()


def test_ecdsa_chosen_scalars(eng, oracle):
    """The construction of test_gpu_keyset_comb.test_ecdsa_chosen_scalars, 256 signatures over 16 keys: u2 at the comb
    recoding's corners with u1 random, u1 = 0 (the generator part is the identity) and R = identity (rejected) - what the lane
    ladder hands to its worklist, the complete formulas decide here."""
    import secp256k1_voi_amd as S
    n, n_keys = 256, 16
    rng = random.Random(2140)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    base = TC.chosen_u2()
    u2 = [base[i % len(base)] for i in range(n)]
    key = [(i // 7) % n_keys for i in range(n)]
    kind = [0 if i < n // 2 else 1 + (i & 1) for i in range(n)]                # 0 random u1, 1 u1 = 0, 2 R = identity
    u1 = [rng.randrange(N) if kd == 0 else 0 if kd == 1 else (-b * d[k]) % N for b, k, kd in zip(u2, key, kind)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    Rp = eng.scalar_base_mult_batch(TC._rows([v or 1 for v in kR]))
    Q = np.ascontiguousarray(eng.scalar_base_mult_batch(TC._rows(d))[:, 1:])
    rr = [int.from_bytes(bytes(Rp[i, 1:33]), "big") % N if kR[i] else rng.randrange(1, N) for i in range(n)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    dig, r, s = TC._rows(ee), TC._rows(rr), TC._rows(ss)
    exp = oracle.ecdsa_verify_batch(np.ascontiguousarray(Q[key]), dig, r, s, nthreads=min(16, os.cpu_count() or 1))
    ok = np.array([kR[i] != 0 and rr[i] != 0 and ss[i] != 0 for i in range(n)])
    assert exp[ok].all() and not exp[~ok].any() and (~ok).sum() >= n // 4
    ks = eng.keyset_create(Q, S.KEYSET_COMB)
    try:
        _row_and_lane(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, np.array(key, np.uint32), dig, r, s), exp)
    finally:
        ks.close()


def test_ecdsa_wrapped_r(eng, oracle):
    """x(R) = r + n with r in [1, p - n): R = (x, y) is chosen with n <= x < p, the key is Q = (R - a G) / b for chosen a, b,
    r = x - n, s = r / b, e = a s.  Valid only through the r + n comparison."""
    import secp256k1_voi_amd as S
    rng = random.Random(2150)
    keys, dig, r, s = [], [], [], []
    x = N
    while len(keys) < 10:
        x += rng.randrange(1, 1 << 100)
        assert x < P
        pt = R.lift_x(x, len(keys) & 1)
        if pt is None:
            continue
        a, b = rng.randrange(1, N), rng.randrange(1, N)
        q = R.mul(pow(b, -1, N), R.add(pt, R.neg(R.mul(a, R.G))))
        rr = x - N
        ss = rr * pow(b, -1, N) % N
        assert 0 < rr < P - N and ss
        keys.append(b32(q[0]) + b32(q[1]))
        dig.append(a * ss % N)
        r.append(rr)
        s.append(ss)
    keys = np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 64).copy()
    dig, r, s = TC._rows(dig), TC._rows(r), TC._rows(s)
    kidx = np.arange(len(keys), dtype=np.uint32)
    assert oracle.ecdsa_verify_batch(keys, dig, r, s, nthreads=1).all()
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        _row_and_lane(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r, s), np.ones(len(keys), np.uint8))
        r2 = r.copy()
        r2[:, 31] ^= 1                                                         # ... and no longer
        _row_and_lane(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r2, s), np.zeros(len(keys), np.uint8))
    finally:
        ks.close()


def _schnorr_batch(eng, oracle, n, nk, seed):
    """n BIP-340 signatures of nk keys over a set of 2 nk + 2 entries: key k as the point with even Y (k even) or odd Y (k odd),
    entry nk + k the OTHER point of the same x (the set lists Q and -Q: either index verifies), then two entries that are no
    keys.  Damage as in test_gpu_keyset_row: s + 1, a longer message, r >= p, an r that does not lift, s >= n, the -R family,
    keys that are none, indices outside the set.  Returns (set keys, kidx, msgs, sig, exp)."""
    rng = random.Random(seed)
    d = [rng.randrange(1, N) for _ in range(nk)]
    key = [i % nk for i in range(n)]
    msgs = [rng.randbytes(KR.MSG_LENGTHS[i % len(KR.MSG_LENGTHS)]) for i in range(n)]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    _, sig_odd, _ = SC.sign(eng, d, key, msgs, rng, odd_nonce=True)
    Pk = eng.scalar_base_mult_batch(SC._rows(d_even))                        # the even-y points
    keys = np.zeros((2 * nk + 2, 64), np.uint8)
    for k in range(nk):
        even = bytes(Pk[k, 1:])
        odd = even[:32] + b32(P - int.from_bytes(even[32:], "big"))
        keys[k] = np.frombuffer(odd if k & 1 else even, np.uint8)
        keys[nk + k] = np.frombuffer(even if k & 1 else odd, np.uint8)
    keys[2 * nk] = np.frombuffer(bytes(Pk[0, 1:33]) + b32((int.from_bytes(bytes(Pk[0, 33:]), "big") + 1) % P), np.uint8)   # not on the curve
    keys[2 * nk + 1] = 0xFF                                                  # coordinates >= p
    x_off = next(x for x in range(2, 100) if R.lift_x(x, 0) is None)
    kidx = [k + nk * ((i // nk) & 1) for i, k in enumerate(key)]             # Q and -Q in turn
    for i in range(n):
        kind = i % 11
        if kind == 1:
            sig[i] = sig[i][:32] + b32((int.from_bytes(sig[i][32:], "big") + 1) % N)
        elif kind == 2:
            msgs[i] = msgs[i] + b"x"
        elif kind == 3:
            sig[i] = b32(P + 5) + sig[i][32:]                                # r >= p
        elif kind == 4:
            sig[i] = b32(x_off) + sig[i][32:]                                # r is no x of the curve
        elif kind == 5:
            sig[i] = sig[i][:32] + b32(N + (i % 3))                          # s >= n
        elif kind == 6:
            sig[i] = sig_odd[i]                                              # -R
        elif kind == 7 and i % 22 == 7:
            kidx[i] = 2 * nk + (i // 22) % 2                                 # a key of the set that is no public key
        elif kind == 8 and i % 22 == 8:
            kidx[i] = (2 * nk + 2, 0xFFFFFFFF)[(i // 22) % 2]                # an index outside the set
    pk = [bytes(keys[k][:32]) if k < 2 * nk + 2 else bytes(32) for k in kidx]
    exp = SC.expected(oracle, pk, msgs, sig)
    exp[[k >= 2 * nk for k in kidx]] = 0
    assert exp[0::11].all() and not exp[6::11].any() and not exp[4::11].any() and 0.3 * n < exp.sum() < 0.6 * n
    return keys, np.array(kidx, np.uint32), msgs, sig, exp


@pytest.fixture(scope="module")
def schnorr_1024(eng, oracle):
    return _schnorr_batch(eng, oracle, 1024, 8, 2160)


def test_schnorr_row_ladder_over_a_comb_set(eng, schnorr_1024):
    """BIP-340, n = 1, 3, 4, 5, 255, 1024 over 8 keys stored with even and with odd Y, each listed as Q and as -Q, ragged
    messages and the damage of _schnorr_batch"""
    import secp256k1_voi_amd as S
    keys, kidx, msgs, sig, exp = schnorr_1024
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        assert ks.valid_keys().tolist() == [1] * 16 + [0, 0]
        for n in SIZES:
            lo = 1024 - n if n < 255 else 0
            sl = slice(lo, lo + n)
            _row_and_lane(eng, lambda: eng.schnorr_verify_batch_keyset(ks, kidx[sl], msgs[sl], sig[sl]), exp[sl])
        # Q and -Q of the same x give the same verdicts
        swapped = np.where(kidx < 8, kidx + 8, np.where(kidx < 16, kidx - 8, kidx)).astype(np.uint32)
        _row_and_lane(eng, lambda: eng.schnorr_verify_batch_keyset(ks, swapped[:255], msgs[:255], sig[:255]), exp[:255])
    finally:
        ks.close()


def test_tickets_and_a_grown_set(eng, ecdsa_1024, schnorr_1024):
    """_submit / wait of both algorithms at n = 255, in flight together (the child contexts inherit the knob), over sets created
    with spare capacity and grown by append: the appended keys verify, an index in n .. cap - 1 gives 0.  A group of one member
    forwards the knob."""
    import secp256k1_voi_amd as S
    keys, kidx, full, dig, r, s, exp = ecdsa_1024
    skeys, skidx, msgs, sig, sexp = schnorr_1024
    n = 255
    eks = eng.keyset_create(keys[:3], S.KEYSET_COMB, capacity=16)
    sks = eng.keyset_create(skeys[:5], S.KEYSET_COMB, capacity=32)
    try:
        assert eks.append(keys[3:]) == 3 and len(eks) == len(keys) and eks.capacity() == 16
        assert sks.append(skeys[5:]) == 5 and len(sks) == len(skeys) and sks.capacity() == 32
        ki = kidx[:n].copy()
        ki[::50] = np.arange(len(ki[::50]), dtype=np.uint32) + len(keys)           # in n .. cap - 1: memory the set has, no key
        assert len(eks) <= ki[::50].min() and ki[::50].max() < eks.capacity()
        e2 = exp[False][:n].copy()
        e2[::50] = 0
        si = skidx[:n].copy()
        si[3::60] = len(skeys) + 1
        s2 = sexp[:n].copy()
        s2[3::60] = 0
        try:
            eng.set_keyset_comb_small_batch_max(KNOB)
            t1 = eng.schnorr_verify_batch_keyset_submit(sks, si, msgs[:n], sig[:n])
            t2 = eng.ecdsa_verify_batch_keyset_submit(eks, ki, dig[:n], r[:n], s[:n])
            assert np.array_equal(t2.wait(), e2) and np.array_equal(t1.wait(), s2)
            eng.wait_all()
        finally:
            eng.set_keyset_comb_small_batch_max(0)
        _row_and_lane(eng, lambda: eng.ecdsa_verify_batch_keyset(eks, ki, dig[:n], r[:n], s[:n]), e2)
        _row_and_lane(eng, lambda: eng.schnorr_verify_batch_keyset(sks, si, msgs[:n], sig[:n]), s2)
    finally:
        eks.close()
        sks.close()
    g = S.Group([0])
    try:
        gks = g.keyset_create(keys, S.KEYSET_COMB)
        try:
            for max_n in (KNOB, 0):
                g.set_keyset_comb_small_batch_max(max_n)
                assert np.array_equal(g.ecdsa_verify_batch_keyset(gks, kidx[:600], dig[:600], r[:600], s[:600]), exp[False][:600]), max_n
        finally:
            gks.close()
    finally:
        g.close()


def test_golden_vectors(eng, oracle):
    """The Wycheproof sha256 vectors (the signatures the oracle's ParseASN1Signature accepts) and the official BIP-340 vectors
    over comb sets of their keys: the vectors' verdicts, which are the plain call's"""
    import secp256k1_voi_amd as S
    H = bytes.fromhex
    items = []
    for c in load_golden("wycheproof_ecdsa_sha256.json")["cases"]:
        rs = oracle.parse_asn1_signature(H(c["sig"]))
        if rs is not None:
            items.append((H(c["pub"])[1:], H(c["digest"])[:32], rs[0], rs[1], int(c["valid"])))
    pub, dig, r, s = (np.frombuffer(b"".join(i[k] for i in items), np.uint8).reshape(len(items), w) for k, w in ((0, 64), (1, 32), (2, 32), (3, 32)))
    exp = np.array([i[4] for i in items], np.uint8)
    assert len(items) <= KNOB and 100 < exp.sum() < len(items)
    assert np.array_equal(eng.ecdsa_verify_batch(pub, dig, r, s), exp)
    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        _row_and_lane(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, inv.reshape(-1).astype(np.uint32), dig, r, s), exp)
    finally:
        ks.close()
    # BIP-340: the vectors' keys as the set (odd y for every other one; keys that do not lift stand in as off-curve points)
    cases = load_golden("bip340.json")["cases"]
    vk = sorted({c["public_key"] for c in cases})
    vkeys = np.zeros((len(vk), 64), np.uint8)
    for j, hx in enumerate(vk):
        pt = R.lift_x(int(hx, 16), j % 2)
        vkeys[j] = np.frombuffer(H(hx) + (b32(pt[1]) if pt else bytes(32)), np.uint8)
    vmsgs, vsigs = [H(c["message"]) for c in cases], [H(c["signature"]) for c in cases]
    vexp = np.array([int(c["valid"]) for c in cases], np.uint8)
    assert np.array_equal(eng.schnorr_verify_batch([H(c["public_key"]) for c in cases], vmsgs, vsigs), vexp)
    ks = eng.keyset_create(vkeys, S.KEYSET_COMB)
    try:
        vidx = np.array([vk.index(c["public_key"]) for c in cases], np.uint32)
        _row_and_lane(eng, lambda: eng.schnorr_verify_batch_keyset(ks, vidx, vmsgs, vsigs), vexp)
    finally:
        ks.close()
