"""Growable key sets (s2k_keyset_create_cap, s2k_keyset_append[_device], s2k_keyset_reserve): a set created with spare
capacity and grown in steps verifies, after every step, exactly as the oracle, the plain call and a set created whole from
all the keys do for the keys it holds, and rejects every signature under an index it does not hold yet; its index follows.

The shapes are the smallest at which a ranged build can go wrong: 37 keys first (a multiple of neither 4 nor 64), then 1, 27,
64 and 71 more (38, 65, 129, 200: around the 64-lane and 256-lane blocks; no section of a set of 200 keys is a multiple of 256
long).  Among the appended keys: one off the curve, one with X >= p, a duplicate of key 5 and the negation of key 7."""
import os

import numpy as np
import pytest

import pyref as R

pytestmark = pytest.mark.gpu
N, P = R.N, R.P
b32 = R.b32
NONE = 0xFFFFFFFF
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768
NKEYS, FIRST, STEPS = 200, 37, (1, 27, 64, 71)
NROW, NSIG = 300, 4096 + 37
OFF_CURVE, BIG_X, DUP, DUP_OF, NEG, NEG_OF = 100, 150, 60, 5, 130, 7
LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _negated(key):
    out = key.copy()
    out[32:] = np.frombuffer(b32(P - int.from_bytes(bytes(key[32:]), "big")), np.uint8)
    return out


def _corrupt(rng, arrays, n):
    """a bit of one of the arrays changed in about a quarter of the n rows"""
    hit = rng.permutation(n)[:n // 4]
    for arr, part in zip(arrays, np.array_split(hit, len(arrays))):
        arr[part, rng.integers(0, arr.shape[1], size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    return hit


@pytest.fixture(scope="module")
def case(eng, oracle):
    """200 keys and 4133 signatures over them (the first 300 are the small call); truth: the oracle and the plain call."""
    from secp256k1_voi_amd.synth import synth_batch
    rng = np.random.default_rng(2301)
    kidx = rng.integers(0, NKEYS, size=NSIG).astype(np.uint32)
    kidx[:8] = [FIRST, FIRST + 1, 65, 129, DUP, NEG, OFF_CURVE, BIG_X]        # (the index n itself at every step, in both calls)
    signer = kidx.copy()                      # the key whose secret signs: the duplicate's and the negation's are their originals'
    signer[kidx == DUP] = DUP_OF
    signer[kidx == NEG] = NEG_OF
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, NKEYS, seed=2302, key_idx=signer))
    Q = np.zeros((NKEYS, 64), np.uint8)
    Q[signer] = pub
    assert set(signer.tolist()) == set(range(NKEYS)) - {DUP, NEG} and len(np.unique(Q, axis=0)) == NKEYS - 1     # (rows DUP and NEG: set below)
    keys = Q.copy()
    keys[OFF_CURVE, 63] ^= 1
    keys[BIG_X, :32] = np.frombuffer(b32(P + 5), np.uint8)
    keys[DUP] = Q[DUP_OF]
    keys[NEG] = _negated(Q[NEG_OF])
    # (r, s) on digest e under Q is (r, s) on digest -e under -Q: u1 G + u2 (-Q) = -(e / s G + r / s Q), the same x
    for i in np.nonzero(kidx == NEG)[0]:
        dig[i] = np.frombuffer(b32((N - int.from_bytes(bytes(dig[i]), "big") % N) % N), np.uint8)
    hit = _corrupt(rng, (r, s, dig), NSIG)
    pub = np.ascontiguousarray(keys[kidx])
    truth = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    assert np.array_equal(eng.ecdsa_verify_batch(pub, dig, r, s), truth)
    clean = np.ones(NSIG, bool)
    clean[hit] = False
    assert not truth[(kidx == OFF_CURVE) | (kidx == BIG_X)].any()
    for k in (DUP, NEG, 0, FIRST, 199):
        sel = clean & (kidx == k)
        assert sel.sum() >= 5 and truth[sel].all(), k                         # they verify as their own keys
    assert 0.6 * NSIG < int(truth.sum()) < 0.8 * NSIG
    valid = np.ones(NKEYS, np.uint8)
    valid[[OFF_CURVE, BIG_X]] = 0
    return dict(keys=keys, valid=valid, kidx=kidx, pub=pub, dig=dig, r=r, s=s, truth=truth)


def _expected(c, live, n=NSIG):
    return np.where(c["kidx"][:n] < live, c["truth"][:n], 0).astype(np.uint8)


def _check_verdicts(eng, S, ks, c, live):
    """both paths over all 200 key indices: the small call (the row ladder, except over a comb set) and the lane path"""
    comb = ks.layout() == S.KEYSET_COMB
    got = eng.ecdsa_verify_batch_keyset(ks, c["kidx"][:NROW], c["dig"][:NROW], c["r"][:NROW], c["s"][:NROW])
    assert eng.last_keyset_ladder() == (S.KEYSET_LADDER_LANE if comb else S.KEYSET_LADDER_ROW)
    exp = _expected(c, live, NROW)
    assert np.array_equal(got, exp), (live, np.nonzero(got != exp)[0][:10])
    got = eng.ecdsa_verify_batch_keyset(ks, c["kidx"], c["dig"], c["r"], c["s"])
    assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
    exp = _expected(c, live)
    assert np.array_equal(got, exp), (live, np.nonzero(got != exp)[0][:10])
    assert not got[c["kidx"] >= live].any() and (c["kidx"] == live).any() == (live < NKEYS)


def _lookup_truth(keys, valid, live, q):
    """the answers of the three lookups for the 64-byte queries q over keys[:live]: the lowest index"""
    d64, d32, d33 = {}, {}, {}
    for i in range(live):
        k = bytes(keys[i])
        d64.setdefault(k, i)
        d32.setdefault(k[:32], i)
        if valid[i]:
            d33.setdefault((k[63] & 1, k[:32]), i)
    e64 = np.array([d64.get(bytes(k), NONE) for k in q], np.uint32)
    e32 = np.array([d32.get(bytes(k[:32]), NONE) for k in q], np.uint32)
    e33 = np.array([d33.get((int(k[63]) & 1, bytes(k[:32])), NONE) for k in q], np.uint32)
    return e64, e32, e33, len(d64)


def _check_index(eng, ks, c, live, queries):
    e64, e32, e33, distinct = _lookup_truth(c["keys"], c["valid"], live, queries)
    assert np.array_equal(eng.keyset_lookup(ks, queries), e64), live
    assert np.array_equal(eng.keyset_lookup(ks, queries, key_bytes=32, stride=64), e32), live
    rec33 = np.ascontiguousarray(np.concatenate([(2 + (queries[:, 63:64] & 1)).astype(np.uint8), queries[:, :32]], axis=1))
    assert np.array_equal(eng.keyset_lookup(ks, rec33, key_bytes=33), e33), live
    assert ks.index_info()["occupied"] == distinct, live


@pytest.fixture(scope="module")
def queries(case):
    keys = case["keys"]
    return np.ascontiguousarray(np.concatenate([keys, np.stack([_negated(k) for k in keys])]))


# ---- 1. stepwise growth, with the index following ----
@pytest.mark.parametrize("log2_slots", [0, 6])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_stepwise_growth(eng, case, queries, layout, log2_slots):
    import secp256k1_voi_amd as S
    c = case
    keys = c["keys"]
    whole = eng.keyset_create(keys, getattr(S, layout))
    ks = eng.keyset_create(keys[:FIRST], getattr(S, layout), capacity=NKEYS)
    try:
        assert whole.layout() == ks.layout() == getattr(S, layout)
        assert len(whole) == whole.capacity() == NKEYS and np.array_equal(whole.valid_keys(), c["valid"])
        assert np.array_equal(eng.ecdsa_verify_batch_keyset(whole, c["kidx"], c["dig"], c["r"], c["s"]), c["truth"])
        assert ks.device_bytes() == whole.device_bytes()                      # what is allocated: for the capacity
        ks.index_create(log2_slots)
        assert ks.index_info()["slots"] == (64 if log2_slots else 512)        # auto: for the capacity
        live = FIRST
        for step in (0,) + STEPS:
            if step:
                assert ks.append(keys[live:live + step]) == live
                live += step
            assert len(ks) == live and ks.capacity() == NKEYS
            assert np.array_equal(ks.valid_keys(), c["valid"][:live])
            _check_verdicts(eng, S, ks, c, live)
            _check_index(eng, ks, c, live, queries)
            # 64 slots hold 38 keys; 65 do not fit: the index is rebuilt at the geometry of the capacity
            assert ks.index_info()["slots"] == (64 if log2_slots and live < 64 else 512)
        assert live == NKEYS and ks.device_bytes() == whole.device_bytes()
        assert ks.append(keys[:0]) == NKEYS                                   # nothing: fine
        with pytest.raises(S.EngineError, match="s2k_keyset_reserve"):
            ks.append(keys[:1])                                               # full
        assert len(ks) == NKEYS
        _check_verdicts(eng, S, ks, c, NKEYS)
        _check_index(eng, ks, c, NKEYS, queries)
        with pytest.raises(S.EngineError):
            eng.keyset_create(keys, getattr(S, layout), capacity=NKEYS - 1)   # a capacity below the keys given
    finally:
        ks.close()
        whole.close()


# ---- 2. reserve ----
@pytest.mark.parametrize("layout", LAYOUTS)
def test_reserve(eng, case, queries, layout):
    import secp256k1_voi_amd as S
    c = case
    keys = c["keys"]
    ks = eng.keyset_create(keys[:FIRST], getattr(S, layout))
    try:
        assert len(ks) == ks.capacity() == FIRST
        before = ks.device_bytes()
        with pytest.raises(S.EngineError, match="s2k_keyset_reserve"):
            ks.append(keys[FIRST:FIRST + 1])                                  # no spare capacity
        for cap in (20, FIRST):
            ks.reserve(cap)
            assert ks.capacity() == FIRST and ks.device_bytes() == before
        ks.index_create()
        assert ks.index_info()["slots"] == 128
        _check_verdicts(eng, S, ks, c, FIRST)
        _check_index(eng, ks, c, FIRST, queries)
        ks.reserve(100)
        assert ks.capacity() == 100 and len(ks) == FIRST and ks.device_bytes() > before
        assert ks.layout() == getattr(S, layout)
        assert ks.index_info()["slots"] == 256                                # 128 < 2 * 100: rebuilt
        assert np.array_equal(ks.valid_keys(), c["valid"][:FIRST])
        _check_verdicts(eng, S, ks, c, FIRST)
        _check_index(eng, ks, c, FIRST, queries)
        assert ks.append(keys[FIRST:100]) == FIRST
        assert len(ks) == 100 and ks.index_info()["slots"] == 256
        _check_verdicts(eng, S, ks, c, 100)
        _check_index(eng, ks, c, 100, queries)
        ks.reserve(129)                                                       # 256 slots are not 2 * 129
        assert ks.index_info()["slots"] == 512
        assert ks.append(keys[100:129]) == 100
        _check_verdicts(eng, S, ks, c, 129)
        _check_index(eng, ks, c, 129, queries)
    finally:
        ks.close()


# ---- 3. the fused calls take the set's tables for appended keys ----
def _lift_even(x32):
    x = int.from_bytes(bytes(x32), "big")
    y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
    assert y * y % P == (x * x * x + 7) % P
    return np.frombuffer(bytes(x32) + b32(y if y % 2 == 0 else P - y), np.uint8)


@pytest.fixture(scope="module")
def fused_case(eng, case):
    """The set of the fused calls: key i of `case` at even i, BIP-340 key i at odd i - so each batch has keys the set will
    never hold.  References: the plain calls on the same arguments."""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_schnorr_batch
    c = case
    pk, msgs, sig = (np.array(a) for a in synth_schnorr_batch(eng, NSIG, NKEYS, seed=2311))
    _corrupt(np.random.default_rng(2312), (sig, msgs), NSIG)
    keys = c["keys"].copy()
    for i in range(1, NKEYS, 2):
        keys[i] = _lift_even(pk[i])
    pubs = [b"\x04" + bytes(q) if k == OFF_CURVE else bytes([2 + (int(q[63]) & 1)]) + bytes(q[:32]) for q, k in zip(c["pub"], c["kidx"])]
    digs = [bytes(d) for d in c["dig"]]
    sigs = [bytes(a) + bytes(b) for a, b in zip(c["r"], c["s"])]
    ref_enc = eng.ecdsa_verify_encoded_batch(pubs, digs, sigs, encoding=S.ENCODING_COMPACT)
    ref_schnorr = eng.schnorr_verify_batch(pk, msgs, sig)
    assert np.array_equal(ref_enc, c["truth"]) and 0.6 * NSIG < int(ref_schnorr.sum()) < 0.8 * NSIG
    valid = c["valid"].copy()
    valid[1::2] = 1
    return dict(keys=keys, valid=valid, pk=pk, msgs=msgs, sig=sig, pubs=pubs, digs=digs, sigs=sigs, ref_enc=ref_enc, ref_schnorr=ref_schnorr)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_calls_follow_appends(eng, case, fused_case, layout):
    import secp256k1_voi_amd as S
    c, f = case, fused_case
    keys = f["keys"]
    ks = eng.keyset_create(keys[:FIRST], getattr(S, layout), capacity=NKEYS)
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    try:
        ks.index_create()
        counts = []
        for live in (FIRST, 129):
            if live > len(ks):
                assert ks.append(keys[len(ks):live]) == FIRST
            held = {bytes(k) for k in keys[:live]}
            held_x = {bytes(k[:32]) for k, v in zip(keys[:live], f["valid"][:live]) if v}
            hits = sum(bytes(q) in held for q in c["pub"])
            hits_x = sum(bytes(x) in held_x for x in f["pk"])
            counts.append((hits, hits_x))
            got = eng.ecdsa_verify_batch_bykey(ks, c["pub"], c["dig"], c["r"], c["s"])
            st = eng.key_grouping_stats()
            assert np.array_equal(got, c["truth"]), live
            assert st["keyed"] == hits and st["general"] == NSIG - hits, (live, st)
            assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
            got = eng.schnorr_verify_batch_bykey(ks, f["pk"], f["msgs"], f["sig"])
            st = eng.key_grouping_stats()
            assert np.array_equal(got, f["ref_schnorr"]), live
            assert st["keyed"] == hits_x and st["general"] == NSIG - hits_x, (live, st)
            got = eng.ecdsa_verify_encoded_batch_keyset(ks, f["pubs"], f["digs"], f["sigs"], encoding=S.ENCODING_COMPACT)
            assert np.array_equal(got, f["ref_enc"]), live
            # the ticket forms
            t1 = eng.ecdsa_verify_batch_bykey_submit(ks, c["pub"], c["dig"], c["r"], c["s"])
            t2 = eng.schnorr_verify_batch_bykey_submit(ks, f["pk"], f["msgs"], f["sig"])
            t3 = eng.ecdsa_verify_encoded_batch_keyset_submit(ks, f["pubs"], f["digs"], f["sigs"], encoding=S.ENCODING_COMPACT)
            assert np.array_equal(t3.wait(), f["ref_enc"]) and np.array_equal(t2.wait(), f["ref_schnorr"])
            assert np.array_equal(t1.wait(), c["truth"])
        # the signatures under the new keys moved from the general ladder to the set's tables
        (h0, x0), (h1, x1) = counts
        assert 0 < h0 < h1 < NSIG and 0 < x0 < x1 < NSIG
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        ks.close()


# ---- 4. append from a device tensor ----
@pytest.mark.parametrize("layout", ["KEYSET_JOINT5", "KEYSET_COMB"])
def test_append_from_device_tensor(eng, case, queries, layout):
    import torch
    import secp256k1_voi_amd as S
    c = case
    keys = c["keys"]
    host = eng.keyset_create(keys[:FIRST], getattr(S, layout), capacity=NKEYS)
    dev = eng.keyset_create(keys[:FIRST], getattr(S, layout), capacity=NKEYS)
    try:
        dev.index_create()
        d_keys = torch.from_numpy(keys[FIRST:]).to(torch.device("cuda", 0))
        assert dev.append(d_keys) == FIRST and host.append(keys[FIRST:]) == FIRST
        assert len(dev) == len(host) == NKEYS
        assert np.array_equal(dev.valid_keys(), host.valid_keys()) and np.array_equal(dev.valid_keys(), c["valid"])
        a = eng.ecdsa_verify_batch_keyset(dev, c["kidx"], c["dig"], c["r"], c["s"])
        b = eng.ecdsa_verify_batch_keyset(host, c["kidx"], c["dig"], c["r"], c["s"])
        assert np.array_equal(a, b) and np.array_equal(a, c["truth"])
        _check_index(eng, dev, c, NKEYS, queries)
        with pytest.raises(ValueError):
            dev.append(torch.zeros(63, dtype=torch.uint8, device=d_keys.device))
    finally:
        host.close()
        dev.close()


# ---- 5. a group's set ----
def test_group_keyset_append(eng, case):
    import secp256k1_voi_amd as S
    c = case
    keys = c["keys"]
    grp = S.Group([0])
    try:
        gks = grp.keyset_create(keys[:FIRST], S.KEYSET_JOINT, capacity=NKEYS)
        assert len(gks) == FIRST and gks.capacity() == NKEYS
        assert np.array_equal(grp.ecdsa_verify_batch_keyset(gks, c["kidx"], c["dig"], c["r"], c["s"]), _expected(c, FIRST))
        assert gks.append(keys[FIRST:129]) == FIRST
        assert len(gks) == 129 and gks.capacity() == NKEYS
        got = grp.ecdsa_verify_batch_keyset(gks, c["kidx"], c["dig"], c["r"], c["s"])
        ks = eng.keyset_create(keys[:129], S.KEYSET_JOINT)
        try:
            assert np.array_equal(got, eng.ecdsa_verify_batch_keyset(ks, c["kidx"], c["dig"], c["r"], c["s"]))
        finally:
            ks.close()
        assert np.array_equal(got, _expected(c, 129))
        with pytest.raises(S.EngineError):
            gks.append(keys[:72])                                             # 129 + 72 > 200
        assert len(gks) == 129
        gks.reserve(201)
        assert gks.capacity() == 201 and gks.append(keys[129:]) == 129 and len(gks) == NKEYS
        assert np.array_equal(grp.ecdsa_verify_batch_keyset(gks, c["kidx"], c["dig"], c["r"], c["s"]), c["truth"])
        gks.close()
    finally:
        grp.close()
