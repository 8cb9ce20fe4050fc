"""Key sets by key bytes: the index of a set (s2k_keyset_index_create: k_ksi_build), the lookup of key bytes in it
(s2k_keyset_lookup[_device]: k_ksi_lookup<64> / <32>) and the ECDSA call that joins them (s2k_ecdsa_verify_batch_keyset_bykey:
lookup, sort, the set's ladder over the hits, k_verify_fast<MODE_ECDSA_LEFT> over the misses, the worklist kernel from the
supplied key bytes).

The lookup is exact against a Python dict (duplicates, Q / -Q pairs, keys that are no public keys, one-bit neighbours, every
alignment path of the loader, a nearly full table); the fused call gives the plain call's and the oracle's verdicts byte for byte
in every layout, with hits and misses counted; exceptional lanes of both kinds end on the worklist; small calls are the plain call."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_comb as TC

pytestmark = pytest.mark.gpu
N = R.N
b32 = R.b32
NONE = 0xFFFFFFFF
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768
NSIG = 4096 + 37


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
    out[32:] = np.frombuffer(b32(R.P - int.from_bytes(bytes(key[32:]), "big")), np.uint8)
    return out


def _truth(keys):
    d64, d32 = {}, {}
    for i, k in enumerate(keys):
        d64.setdefault(bytes(k), i)
        d32.setdefault(bytes(k[:32]), i)
    return d64, d32


# ---- 1. the lookup is exact ----
@pytest.fixture(scope="module")
def lookup_case(eng):
    """1000 keys: 948 real ones, the negations of 10 of them, 40 duplicates (of plain keys, of both halves of a pair, of the key
    that is off the curve), one key off the curve, one with X >= p; in a shuffled order.  5000 queries: hits, random strings, and
    keys of the set with one bit of the last byte of Y or of the first byte of X changed."""
    from secp256k1_voi_amd.synth import synth_batch
    rng = np.random.default_rng(1901)
    pool = np.array(synth_batch(eng, 960, 960, seed=1902)[0])
    assert len(np.unique(pool, axis=0)) == 960
    real, extra = pool[:948], pool[948:]
    negs = np.stack([_negated(k) for k in real[100:110]])
    off = extra[0].copy()
    off[63] ^= 1                                                              # off the curve
    big = extra[1].copy()
    big[:32] = np.frombuffer(b32(R.P + 5), np.uint8)                          # X >= p: not canonical
    first = np.concatenate([real, negs, off[None], big[None]])
    dup_of = np.concatenate([rng.integers(0, 948, size=36), [100, 948, 958, 959]])     # (948: the negation of key 100)
    keys = np.concatenate([first, first[dup_of]])
    keys = np.ascontiguousarray(keys[rng.permutation(len(keys))])
    assert keys.shape == (1000, 64)
    d64, d32 = _truth(keys)
    assert len(d64) == 960 and len(d32) == 950
    nq = 5000
    q = keys[rng.integers(0, 1000, size=nq)].copy()
    kind = rng.permutation(nq) % 10                                           # 0-5 hit, 6-7 random, 8 Y neighbour, 9 X neighbour
    q[kind == 6] = rng.integers(0, 256, size=(int((kind == 6).sum()), 64), dtype=np.uint8)
    q[kind == 7] = rng.integers(0, 256, size=(int((kind == 7).sum()), 64), dtype=np.uint8)
    i8, i9 = np.nonzero(kind == 8)[0], np.nonzero(kind == 9)[0]
    q[i8, 63] ^= (1 << rng.integers(0, 8, size=i8.size)).astype(np.uint8)
    q[i9, 0] ^= (1 << rng.integers(0, 8, size=i9.size)).astype(np.uint8)
    kind[0] = 0                                                               # (the call of one key: a hit)
    q[0] = keys[999]
    exp64 = np.array([d64.get(bytes(k), NONE) for k in q], np.uint32)
    exp32 = np.array([d32.get(bytes(k[:32]), NONE) for k in q], np.uint32)
    assert (exp64[kind < 6] != NONE).all() and (exp64[kind >= 6] == NONE).all()
    assert (exp32[kind == 8] != NONE).all() and (exp32[(kind == 6) | (kind == 7) | (kind == 9)] == NONE).all()
    return keys, q, exp64, exp32, len(d64)


@pytest.mark.parametrize("log2_slots", [0, 10])
def test_lookup_is_exact(eng, lookup_case, log2_slots):
    import torch
    import secp256k1_voi_amd as S
    keys, q, exp64, exp32, distinct = lookup_case
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        bytes_before = ks.device_bytes()
        assert ks.index_info() == dict(slots=0, bytes=0, occupied=0, longest_probe=0)
        ks.index_create(log2_slots)
        info = ks.index_info()
        assert (info["slots"], info["bytes"]) == S.keyset_index_geometry(1000, log2_slots)
        assert info["slots"] == (1024 if log2_slots else 2048) and info["occupied"] == distinct
        assert 0 < info["longest_probe"] < info["slots"]
        assert ks.device_bytes() == bytes_before                              # (the index is an allocation of its own)
        for n in (1, 257, 5000):
            qq = np.ascontiguousarray(q[:n])
            assert np.array_equal(eng.keyset_lookup(ks, qq), exp64[:n]), n
            assert np.array_equal(eng.keyset_lookup(ks, np.ascontiguousarray(qq[:, :32]), key_bytes=32), exp32[:n]), n
            assert np.array_equal(eng.keyset_lookup(ks, qq, key_bytes=32, stride=64), exp32[:n]), n
            rec65 = np.concatenate([np.full((n, 1), 4, np.uint8), qq], axis=1)          # 04 || X || Y, read from offset 1
            assert np.array_equal(eng.keyset_lookup(ks, rec65, key_bytes=64, stride=65, offset=1), exp64[:n]), n
            assert np.array_equal(eng.keyset_lookup(ks, rec65, key_bytes=32, stride=65, offset=1), exp32[:n]), n
            rec68 = np.concatenate([np.zeros((n, 4), np.uint8), qq], axis=1)            # word-aligned, not quad-aligned
            assert np.array_equal(eng.keyset_lookup(ks, rec68, key_bytes=64, stride=68, offset=4), exp64[:n]), n
            assert np.array_equal(eng.keyset_lookup(ks, rec68, key_bytes=32, stride=68, offset=4), exp32[:n]), n
        # the device form, on 65-byte records
        dev = torch.device("cuda", 0)
        n = 5000
        d_rec = torch.from_numpy(np.concatenate([np.full((n, 1), 4, np.uint8), q], axis=1)).to(dev)
        d_out = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.keyset_lookup_device(ks, n, d_rec.data_ptr() + 1, d_out.data_ptr(), key_bytes=64, stride=65)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), exp64)
        assert eng.keyset_lookup(ks, np.zeros((0, 64), np.uint8)).shape == (0,)
    finally:
        ks.close()


def test_lookup_one_key_two_slots(eng, lookup_case):
    import secp256k1_voi_amd as S
    keys, q, _, _, _ = lookup_case
    ks = eng.keyset_create(keys[:1], S.KEYSET_CHUNKS)
    try:
        ks.index_create(1)
        assert ks.index_info() == dict(slots=2, bytes=16, occupied=1, longest_probe=0)
        qq = np.ascontiguousarray(np.concatenate([keys[:1], q[:300], keys[:1], _negated(keys[0])[None]]))
        exp = np.array([0 if bytes(k) == bytes(keys[0]) else NONE for k in qq], np.uint32)
        exp_x = np.array([0 if bytes(k[:32]) == bytes(keys[0, :32]) else NONE for k in qq], np.uint32)
        assert np.array_equal(eng.keyset_lookup(ks, qq), exp) and exp[0] == 0 and exp[-1] == NONE and exp[-2] == 0
        assert np.array_equal(eng.keyset_lookup(ks, qq, key_bytes=32, stride=64), exp_x) and exp_x[-1] == 0
    finally:
        ks.close()


# ---- 2. fused verdicts ----
@pytest.fixture(scope="module")
def fused_case(eng, oracle):
    """4096 + 37 signatures of 80 keys, a tenth damaged; keys 3 and 7 (in the set: the first 64) and key 70 (outside) are no
    public keys.  Reference verdicts: the plain call under the same settings (thresholds off) and the oracle, per flag."""
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, 80, seed=1911))
    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    keys, inv = keys.copy(), inv.reshape(-1)
    assert len(keys) == 80
    keys[3, 63] ^= 1                                                                    # off the curve
    keys[7, :32] = np.frombuffer(b32(R.P + 5), np.uint8)                                # x >= p: not canonical
    keys[70, 63] ^= 1
    pub = np.ascontiguousarray(keys[inv])
    rng = np.random.default_rng(1912)
    hit = rng.permutation(NSIG)[:NSIG // 10]
    for arr, part in zip((r, s, dig), np.array_split(hit, 3)):
        arr[part, rng.integers(0, 32, size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    # half of the valid signatures with the high s: the low-s rule has something to reject
    flip = np.nonzero(np.arange(NSIG) % 2 == 1)[0]
    s[flip] = TC._rows([(N - int.from_bytes(bytes(x), "big")) % N for x in s[flip]])
    other = np.unique(np.array(synth_batch(eng, 64, 64, seed=1913)[0]), axis=0)
    ref, exp = {}, {}
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    try:
        for rm in (False, True):
            ref[rm] = eng.ecdsa_verify_batch(pub, dig, r, s, reject_malleable=rm)
            exp[rm] = oracle.ecdsa_verify_batch(pub, dig, r, s, reject_malleable=rm, nthreads=os.cpu_count() or 1)
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
    assert np.array_equal(ref[False], exp[False]) and np.array_equal(ref[True], exp[True])
    assert not ref[False][(inv == 3) | (inv == 7) | (inv == 70)].any()
    assert 0.7 * NSIG < int(ref[False].sum()) < NSIG and 0.3 * NSIG < int(ref[True].sum()) < 0.6 * NSIG
    return dict(pub=pub, dig=dig, r=r, s=s, keys=keys, inv=inv, other=other, ref=ref)


LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_verdicts(eng, fused_case, layout):
    import secp256k1_voi_amd as S
    c = fused_case
    pub, dig, r, s, inv = c["pub"], c["dig"], c["r"], c["s"], c["inv"]
    in_set = int((inv < 64).sum())
    sets = []
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    try:
        for keys, hits in ((c["keys"][:64], in_set), (c["other"], 0), (c["keys"], NSIG)):
            ks = eng.keyset_create(keys, getattr(S, layout))
            sets.append(ks)
            assert ks.layout() == getattr(S, layout)
            ks.index_create()
            for rm in (False, True):
                got = eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s, reject_malleable=rm)
                st = eng.key_grouping_stats()
                assert np.array_equal(got, c["ref"][rm]), (len(keys), rm, np.nonzero(got != c["ref"][rm])[0][:10])
                assert st["keyed"] == hits and st["general"] == NSIG - hits and st["tables"] == 0, st
                assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
            assert 0.7 * NSIG < int(eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s).sum()) < NSIG
        # every signature that is not decided before the ladder (a key that is none, r or s out of range) through the worklist
        # kernel: more than either side alone has, so it read the supplied key bytes for hits and for misses
        got = eng.ecdsa_verify_batch_bykey(sets[0], pub, dig, r, s, force_worklist=True)
        assert np.array_equal(got, c["ref"][False])
        assert max(in_set, NSIG - in_set) < eng.key_grouping_stats()["complete"] <= NSIG
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        for ks in sets:
            ks.close()


# ---- 3. exceptional lanes from both sides ----
def test_exceptional_lanes_among_hits_and_misses(eng, oracle):
    """test_gpu_keyset_comb.test_ecdsa_chosen_scalars at 1024 signatures over 16 keys, 8 of them in the set: u1 = 0 lanes (the
    generator part is the identity: the worklist's) and R = identity lanes (rejected) among the hits and among the misses"""
    import secp256k1_voi_amd as S
    n, n_keys = 1024, 16
    rng = random.Random(1921)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    base = TC.chosen_u2()
    u2 = [base[i % len(base)] for i in range(n)]
    key = [i % n_keys for i in range(n)]
    kind = [0 if i < n // 2 else 1 + ((i // n_keys) & 1) for i in range(n)]            # 0 random u1, 1 u1 = 0, 2 R = identity
    u1 = [rng.randrange(N) if kd == 0 else 0 if kd == 1 else (-b * d[k]) % N for b, k, kd in zip(u2, key, kind)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    Rp = eng.scalar_base_mult_batch(TC._rows([v or 1 for v in kR]))
    Q = np.ascontiguousarray(eng.scalar_base_mult_batch(TC._rows(d))[:, 1:])
    rr = [int.from_bytes(bytes(Rp[i, 1:33]), "big") % N if kR[i] else rng.randrange(1, N) for i in range(n)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    dig, r, s = TC._rows(ee), TC._rows(rr), TC._rows(ss)
    pub = np.ascontiguousarray(Q[key])
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    kinds, in_set = np.array(kind), np.array(key) < 8
    for side in (in_set, ~in_set):                                                       # both kinds on both sides
        assert (kinds[side] == 1).sum() >= n // 16 and (kinds[side] == 2).sum() >= n // 16
    ok = np.array([kR[i] != 0 and rr[i] != 0 and ss[i] != 0 for i in range(n)])
    assert exp[ok].all() and not exp[~ok].any() and (~ok).sum() >= n // 4
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    sets = []
    try:
        for layout in (S.KEYSET_COMB, S.KEYSET_JOINT5):
            ks = eng.keyset_create(Q[:8], layout)
            sets.append(ks)
            ks.index_create()
            got = eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s)
            st = eng.key_grouping_stats()
            assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
            assert st["keyed"] == int(in_set.sum()) and st["general"] == int((~in_set).sum())
            assert st["complete"] >= int((kinds == 1).sum()), "the u1 = 0 lanes of both sides are the worklist's"
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        for ks in sets:
            ks.close()


# ---- 4. delegation and errors ----
def test_delegation_and_errors(eng, fused_case):
    import torch
    import secp256k1_voi_amd as S
    c = fused_case
    n = 1000
    pub, dig, r, s = (np.ascontiguousarray(c[k][:n]) for k in ("pub", "dig", "r", "s"))
    ks = eng.keyset_create(c["keys"][:64], S.KEYSET_COMB)
    bare = eng.keyset_create(c["keys"][:64], S.KEYSET_COMB)
    other_eng = S.Engine(0)
    try:
        ks.index_create()
        # default thresholds: a call of 1000 signatures IS the plain call (no grouping, no worklist)
        got = eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s)
        st = eng.key_grouping_stats()
        assert np.array_equal(got, eng.ecdsa_verify_batch(pub, dig, r, s)) and np.array_equal(got, c["ref"][False][:n])
        assert st == dict(keyed=0, tables=0, general=0, complete=0), st
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(x).to(dev) for x in (pub, dig, r, s)]
        out = torch.zeros(n, dtype=torch.uint8, device=dev)
        eng.ecdsa_verify_batch_bykey_device(ks, n, *(x.data_ptr() for x in t), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got)
        assert eng.ecdsa_verify_batch_bykey(ks, pub[:0], dig[:0], r[:0], s[:0]).shape == (0,)
        # refusals
        with pytest.raises(S.EngineError):
            eng.ecdsa_verify_batch_bykey(bare, pub, dig, r, s)                         # no index: never built implicitly
        with pytest.raises(S.EngineError):
            eng.keyset_lookup(bare, pub)
        assert bare.index_info()["slots"] == 0
        with pytest.raises(S.EngineError):
            ks.index_create()                                                          # a set has one index
        with pytest.raises(S.EngineError):
            bare.index_create(6)                                                       # 64 slots for 64 keys
        with pytest.raises(S.EngineError):
            bare.index_create(32)
        assert bare.index_info()["slots"] == 0
        bare.index_create(7)
        assert bare.index_info()["slots"] == 128 and np.array_equal(eng.keyset_lookup(bare, pub), eng.keyset_lookup(ks, pub))
        with pytest.raises(S.EngineError):
            other_eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s)                     # a set of another engine
        with pytest.raises(S.EngineError):
            other_eng.keyset_lookup(ks, pub)
        with pytest.raises(S.EngineError):
            eng.ecdsa_verify_batch_bykey_device(ks, n, *(x.data_ptr() for x in t), out.data_ptr(), flags=S.FORCE_COMPLETE)
        with pytest.raises(S.EngineError):
            eng.keyset_lookup_device(ks, n, t[0].data_ptr(), out.data_ptr(), key_bytes=48)
        with pytest.raises(ValueError):
            eng.ecdsa_verify_batch_bykey(ks, pub[:-1], dig, r, s)
        with pytest.raises(ValueError):
            eng.keyset_lookup(ks, pub, key_bytes=48)
    finally:
        other_eng.close()
        bare.close()
        ks.close()
