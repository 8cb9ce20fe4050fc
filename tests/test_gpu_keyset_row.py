"""Small calls over a key set: the wave-per-signature ladder on the set's 32-chunk tables (small_call.hip: k_verify_row_keyset,
k_schnorr_row_keyset; fe29r.h: pt29r_add_b3 on the key's isomorphic curve y^2 = x^3 + 7 W^6).

Every verdict is compared three ways: with the CPU oracle's on the expanded keys (pyref / the oracle's schnorr_verify for
BIP-340), with the same call on the lane-per-signature path (set_keyset_small_batch_max(0)), and last_keyset_ladder() says
which of the two ran.  The addition itself runs through the C-ABI (S2K_HP_PT29R_ADD_B3) against the affine group law."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_comb as TC
import test_gpu_schnorr_comb as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
N, P = R.N, R.P
b32 = R.b32
SIZES = (1, 3, 4, 5, 255, 1024)       # a lone wave, a partial block, a whole block, a block and a wave, many blocks
DEFAULT_MAX = 2048                    # what a new context starts with (s2k_ctx_set_keyset_small_batch_max)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _ints(a):
    return [int.from_bytes(bytes(x), "big") for x in np.asarray(a)]


def _three_ways(eng, call, exp, expect_row=True):
    """call() with the row ladder on and off: both give `exp`; last_keyset_ladder() names the ladder each time"""
    import secp256k1_voi_amd as S
    try:
        eng.set_keyset_small_batch_max(3072)
        got = call()
        assert eng.last_keyset_ladder() == (S.KEYSET_LADDER_ROW if expect_row else S.KEYSET_LADDER_LANE)
        if expect_row:
            assert eng.key_grouping_stats() == {"keyed": 0, "tables": 0, "general": 0, "complete": 0}
        eng.set_keyset_small_batch_max(0)
        lane = call()
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
    finally:
        eng.set_keyset_small_batch_max(DEFAULT_MAX)
    assert np.array_equal(got, exp), np.nonzero(np.asarray(got) != np.asarray(exp))[0][:10]
    assert np.array_equal(lane, exp), np.nonzero(np.asarray(lane) != np.asarray(exp))[0][:10]
    return got


def test_new_symbols_and_defaults(eng):
    import secp256k1_voi_amd as S
    assert (S.KEYSET_LADDER_LANE, S.KEYSET_LADDER_ROW) == (0, 1) and S.HP_PT29R_ADD_B3 == S.HP_XYZZ_ADD_FIRST + 1
    from secp256k1_voi_amd.synth import synth_batch
    e2 = S.Engine(0)
    try:
        assert e2.last_keyset_ladder() == -1
        n = DEFAULT_MAX + 1                                   # the default threshold: at most 3072, the measured crossover
        pub, dig, r, s = (np.array(a) for a in synth_batch(e2, n, 1, seed=1405))
        ks = e2.keyset_create(pub[:1], S.KEYSET_CHUNKS)
        try:
            zeros = np.zeros(n, np.uint32)
            assert e2.ecdsa_verify_batch_keyset(ks, zeros[:-1], dig[:-1], r[:-1], s[:-1]).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_ROW
            assert e2.ecdsa_verify_batch_keyset(ks, zeros, dig, r, s).all() and e2.last_keyset_ladder() == S.KEYSET_LADDER_LANE
        finally:
            ks.close()
    finally:
        e2.close()


@pytest.mark.parametrize("ylazy", [0, 1])
def test_pt29r_add_b3_op(eng, ylazy):
    """S2K_HP_PT29R_ADD_B3 on 64 items: P and Q of secp256k1 moved to y^2 = x^3 + 7 W^6 for a random W, added there with
    b3 = 21 W^6, and moved back: P + Q (chained: P + 17 Q) of the affine law.  P = Q, P = -Q, the identity as P, as Q and as
    both ((0, 0) stands for it), both lazy codes of y; flag 2 would mean the four rows of a wave disagree."""
    import secp256k1_voi_amd as S
    rnd = random.Random(1410 + ylazy)
    n = 64
    pts = [R.mul(rnd.randrange(1, N), R.G) for _ in range(n)]
    qs = [R.mul(rnd.randrange(1, N), R.G) for _ in range(n)]
    for i in range(n):
        kind = i % 8
        if kind == 1:
            qs[i] = pts[i]
        elif kind == 2:
            qs[i] = R.neg(pts[i])
        elif kind == 3:
            pts[i] = None
        elif kind == 4:
            qs[i] = None
        elif kind == 5 and i % 16 == 5:
            pts[i] = qs[i] = None
    w = [rnd.randrange(1, P) for _ in range(n)]
    w[0], w[6] = 1, P - 1
    xy = lambda pt: pt if pt is not None else (0, 0)
    cols = [[b32(xy(p)[0]) for p in pts], [b32(xy(p)[1]) for p in pts], [b32(v) for v in w],
            [b32(xy(q)[0]) for q in qs], [b32(xy(q)[1]) for q in qs]]
    for reps in (1, 17):
        x, y, flag = eng.fp_op_batch_ex(S.HP_PT29R_ADD_B3, cols, ylazy | reps << 20)
        for i, (xi, yi, f) in enumerate(zip(_ints(x), _ints(y), flag)):
            e = pts[i]
            for _ in range(reps):
                e = R.add(e, qs[i])
            if e is None:
                assert f == 0, (i, reps, f)
            else:
                assert f == 1 and (xi, yi) == e, (i, reps, f)


def _ecdsa_batch(eng, n, n_keys, seed):
    """n signatures of n_keys keys (+ two set entries that are no keys), a tenth damaged in r, s or the digest, some indices
    outside the set, every ninth signature with high s: (keys, kidx, full keys, dig, r, s)"""
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, n, n_keys, seed=seed))
    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    kidx = inv.reshape(-1).astype(np.uint32)
    bad = keys[:2].copy()
    bad[0, 63] ^= 1                                                          # off the curve
    bad[1, :32] = np.frombuffer(b32(P + 5), np.uint8)                        # x >= p: not canonical
    keys = np.concatenate([keys, bad])
    rng = np.random.default_rng(seed + 1)
    for i in range(0, n, 9):                                                 # high s: (r, n - s) verifies too, unless rejected
        s[i] = np.frombuffer(b32(N - int.from_bytes(bytes(s[i]), "big")), np.uint8)
    hit = rng.permutation(n)[:max(n // 10, 1 if n > 2 else 0)]
    for arr, part in zip((r, s, dig), np.array_split(hit, 3)):
        arr[part, rng.integers(0, 32, size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    if n >= 5:
        for j, i in enumerate(range(4, n, 37)):
            kidx[i] = (len(keys), 0xFFFFFFFF, len(keys) - 1, len(keys) - 2)[j % 4]   # outside twice; the two that are no keys
    inside = kidx < len(keys)
    full = np.zeros((n, 64), np.uint8)
    full[inside] = keys[kidx[inside]]
    return keys, kidx, full, dig, r, s


@pytest.fixture(scope="module")
def ecdsa_1024(eng, oracle):
    keys, kidx, full, dig, r, s = _ecdsa_batch(eng, 1024, 8, 1420)
    exp = {rm: oracle.ecdsa_verify_batch(full, dig, r, s, reject_malleable=rm, nthreads=min(16, os.cpu_count() or 1)) for rm in (False, True)}
    assert 0 < exp[True].sum() < exp[False].sum() < 1024
    return keys, kidx, full, dig, r, s, exp


@pytest.mark.parametrize("layout", [1, 2, 3, 4])
def test_ecdsa_row_ladder_all_layouts(eng, ecdsa_1024, layout):
    """Sets of layout CHUNKS, JOINT, JOINT5, JOINT6 (all keep the chunk table), n = 1, 3, 4, 5, 255, 1024: the oracle's verdicts
    on the expanded keys, the lane path's, and ROW / LANE reported.  Fails on a library without the row ladder."""
    keys, kidx, full, dig, r, s, exp = ecdsa_1024
    ks = eng.keyset_create(keys, layout)
    try:
        assert ks.layout() == layout and ks.valid_keys().tolist() == [1] * (len(keys) - 2) + [0, 0]
        for n in SIZES:
            lo = 1024 - n if n < 255 else 0                                   # (small slices from the end, large from the start)
            sl = slice(lo, lo + n)
            for rm in (False, True):
                got = _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx[sl], dig[sl], r[sl], s[sl], reject_malleable=rm), exp[rm][sl])
            if n == 1024:
                outside = kidx >= len(keys) - 2
                assert outside.sum() >= 8 and not got[outside].any()
    finally:
        ks.close()


def test_one_key_and_duplicate_key_sets(eng, oracle):
    from secp256k1_voi_amd.synth import synth_batch
    import secp256k1_voi_amd as S
    n = 300
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, n, 1, seed=1431))
    s[::5, 9] ^= 0x20
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=min(16, os.cpu_count() or 1))
    assert exp.sum() == n - len(range(0, n, 5))
    one = eng.keyset_create(pub[:1], S.KEYSET_CHUNKS)
    try:
        _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(one, np.zeros(n, np.uint32), dig, r, s), exp)
    finally:
        one.close()
    other = np.array(synth_batch(eng, 1, 1, seed=1432)[0])
    dup = eng.keyset_create(np.concatenate([pub[:1], other, pub[:1], pub[:1]]), S.KEYSET_JOINT)
    try:
        kidx = np.array([(0, 2, 3, 1)[i % 4] for i in range(n)], np.uint32)
        e2 = exp.copy()
        e2[kidx == 1] = 0
        _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(dup, kidx, dig, r, s), e2)
    finally:
        dup.close()


def test_ecdsa_chosen_scalars(eng, oracle):
    """The construction of test_gpu_keyset_comb.test_ecdsa_chosen_scalars, 256 signatures over 16 keys: u2 at the recoding's
    corners with u1 random, u1 = 0 (the generator part is the identity) and R = identity (rejected) - what the lane ladders
    hand to the worklist, the complete formulas decide here."""
    import secp256k1_voi_amd as S
    n, n_keys = 256, 16
    rng = random.Random(1441)
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
    for layout in (S.KEYSET_CHUNKS, S.KEYSET_JOINT5):
        ks = eng.keyset_create(Q, layout)
        try:
            _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, np.array(key, np.uint32), dig, r, s), exp)
        finally:
            ks.close()


def test_ecdsa_wrapped_r(eng, oracle):
    """x(R) = r + n with r in [1, p - n): R = (x, y) is chosen with n <= x < p, the key is Q = (R - a G) / b for chosen a, b
    (so R = a G + b Q with u1 = a, u2 = b known), r = x - n, s = r / b, e = a s.  Valid only through the r + n comparison."""
    import secp256k1_voi_amd as S
    rng = random.Random(1451)
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
    exp = oracle.ecdsa_verify_batch(keys, dig, r, s, nthreads=1)
    assert exp.all()
    ks = eng.keyset_create(keys, S.KEYSET_CHUNKS)
    try:
        _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r, s), exp)
        r2 = r.copy()
        r2[:, 31] ^= 1                                                         # ... and no longer
        _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r2, s), np.zeros(len(keys), np.uint8))
    finally:
        ks.close()


MSG_LENGTHS = (0, 1, 32, 33, 64, 100)


@pytest.mark.parametrize("layout", [1, 3])
def test_schnorr_row_ladder(eng, oracle, layout):
    """BIP-340 over sets of layout CHUNKS and JOINT5, n = 1, 5, 300: half the set's keys stored with odd Y, ragged messages,
    r not on the curve, r >= p, s >= n, a wrong message, the -R family (the equation holds, y(R) is odd: rejected), keys of the
    set that are none and indices outside it."""
    rng = random.Random(1461 + layout)
    n, nk = 300, 12
    d = [rng.randrange(1, N) for _ in range(nk)]
    key = [i % nk for i in range(n)]
    msgs = [rng.randbytes(MSG_LENGTHS[i % len(MSG_LENGTHS)]) for i in range(n)]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    _, sig_odd, _ = SC.sign(eng, d, key, msgs, rng, odd_nonce=True)
    Pk = eng.scalar_base_mult_batch(SC._rows(d_even))                        # the even-y points
    keys = np.zeros((nk + 2, 64), np.uint8)
    keys[:nk] = Pk[:, 1:]
    for k in range(1, nk, 2):                                               # every other key: the point with the OTHER y
        keys[k, 32:] = np.frombuffer(b32(P - int.from_bytes(bytes(Pk[k, 33:]), "big")), np.uint8)
    keys[nk] = np.frombuffer(bytes(Pk[0, 1:33]) + b32((int.from_bytes(bytes(Pk[0, 33:]), "big") + 1) % P), np.uint8)   # not on the curve
    keys[nk + 1] = 0xFF                                                      # coordinates >= p
    x_off = next(x for x in range(2, 100) if R.lift_x(x, 0) is None)
    kidx = list(key)
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
            kidx[i] = nk + (i // 22) % 2                                     # a key of the set that is no public key
        elif kind == 8 and i % 22 == 8:
            kidx[i] = (nk + 2, 0xFFFFFFFF)[(i // 22) % 2]                    # an index outside the set
    pk = [bytes(keys[k][:32]) if k < nk + 2 else bytes(32) for k in kidx]
    exp = SC.expected(oracle, pk, msgs, sig)
    exp[[k >= nk for k in kidx]] = 0
    assert exp[0::11].all() and not exp[6::11].any() and 0.3 * n < exp.sum() < 0.6 * n
    ks = eng.keyset_create(keys, layout)
    try:
        assert ks.layout() == layout and ks.valid_keys().tolist() == [1] * nk + [0, 0]
        for m in (1, 5, 300):
            lo = 0 if m == 300 else 3
            sl = slice(lo, lo + m)
            _three_ways(eng, lambda: eng.schnorr_verify_batch_keyset(ks, np.array(kidx[sl], np.uint32), msgs[sl], sig[sl]), exp[sl])
    finally:
        ks.close()
    # the official vectors, their keys as the set (odd y for every other one; keys that do not lift stand in as off-curve points)
    H = bytes.fromhex
    cases = load_golden("bip340.json")["cases"]
    vk = sorted({c["public_key"] for c in cases})
    vkeys = np.zeros((len(vk), 64), np.uint8)
    for j, hx in enumerate(vk):
        pt = R.lift_x(int(hx, 16), j % 2)
        vkeys[j] = np.frombuffer(H(hx) + (b32(pt[1]) if pt else bytes(32)), np.uint8)
    ks = eng.keyset_create(vkeys, layout)
    try:
        vidx = np.array([vk.index(c["public_key"]) for c in cases], np.uint32)
        _three_ways(eng, lambda: eng.schnorr_verify_batch_keyset(ks, vidx, [H(c["message"]) for c in cases], [H(c["signature"]) for c in cases]),
                    np.array([int(c["valid"]) for c in cases], np.uint8))
    finally:
        ks.close()


def test_comb_set_keeps_the_lane_path(eng, ecdsa_1024):
    import secp256k1_voi_amd as S
    keys, kidx, full, dig, r, s, exp = ecdsa_1024
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        _three_ways(eng, lambda: eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r, s), exp[False], expect_row=False)
    finally:
        ks.close()


def test_force_worklist_keeps_its_meaning(eng, ecdsa_1024):
    """S2K_ECDSA_FORCE_WORKLIST sends every lane of the lane-per-signature ladder to the complete-formula kernel: such a call
    stays on that path whatever its size"""
    import secp256k1_voi_amd as S
    keys, kidx, full, dig, r, s, exp = ecdsa_1024
    ks = eng.keyset_create(keys, S.KEYSET_CHUNKS)
    try:
        pick = np.nonzero(kidx < len(keys) - 2)[0][:256]                       # (signatures that name a key reach the ladder)
        got = eng.ecdsa_verify_batch_keyset(ks, kidx[pick], dig[pick], r[pick], s[pick], force_worklist=True)
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE and eng.key_grouping_stats()["complete"] == 256
        assert np.array_equal(got, exp[False][pick])
    finally:
        ks.close()


def test_tickets_and_group(eng, oracle, ecdsa_1024):
    """One ECDSA and one BIP-340 key-set ticket of 300 items in flight together give the synchronous calls' verdicts (the child
    contexts inherit the setting); a group of one member with the setting forwarded does the same for a 600-item call."""
    import secp256k1_voi_amd as S
    keys, kidx, full, dig, r, s, exp = ecdsa_1024
    rng = random.Random(1471)
    n, nk = 300, 6
    d = [rng.randrange(1, N) for _ in range(nk)]
    key = [i % nk for i in range(n)]
    msgs = [rng.randbytes(MSG_LENGTHS[i % len(MSG_LENGTHS)]) for i in range(n)]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    for i in range(0, n, 4):
        msgs[i] = msgs[i] + b"!"
    skeys = np.ascontiguousarray(eng.scalar_base_mult_batch(SC._rows(d))[:, 1:])         # (as given: some with odd Y)
    sexp = SC.expected(oracle, pk, msgs, sig)
    assert 0 < sexp.sum() < n
    eks = eng.keyset_create(keys, S.KEYSET_JOINT)
    sks = eng.keyset_create(skeys, S.KEYSET_CHUNKS)
    try:
        t1 = eng.schnorr_verify_batch_keyset_submit(sks, np.array(key, np.uint32), msgs, sig)
        t2 = eng.ecdsa_verify_batch_keyset_submit(eks, kidx[:n], dig[:n], r[:n], s[:n])
        assert np.array_equal(t2.wait(), exp[False][:n]) and np.array_equal(t1.wait(), sexp)
        eng.wait_all()
        assert np.array_equal(eng.schnorr_verify_batch_keyset(sks, np.array(key, np.uint32), msgs, sig), sexp)
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_ROW
    finally:
        eks.close()
        sks.close()
    g = S.Group([0])
    try:
        gks = g.keyset_create(keys, S.KEYSET_CHUNKS)
        try:
            for max_n in (DEFAULT_MAX, 0):
                g.set_keyset_small_batch_max(max_n)
                assert np.array_equal(g.ecdsa_verify_batch_keyset(gks, kidx[:600], dig[:600], r[:600], s[:600]), exp[False][:600]), max_n
        finally:
            gks.close()
    finally:
        g.close()
