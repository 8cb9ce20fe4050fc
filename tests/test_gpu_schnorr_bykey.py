"""BIP-340 over a key set by x-only key bytes (s2k_schnorr_verify_batch_keyset_bykey[_device|_submit]: the valid-only lookup
k_ksi_lookup<S2K_KSI_X_VALID>, the sort, the set's ladder over the hits, k_verify_fast<MODE_SCHNORR_LEFT> over the misses,
finish and worklist kernels on the caller's key bytes) and the ticket form of the ECDSA call by key bytes
(s2k_ecdsa_verify_batch_keyset_bykey_submit).

The fused call gives s2k_schnorr_verify_batch's and the oracle's verdicts byte for byte in every layout of the set, with hits and
misses counted; a key the set lists only as an entry that is no point is a miss and verifies (the lookup with key_bytes 32 in
front of the by-index call rejects it); exceptional lanes of both sides end on the worklist; small calls are the plain call;
device form and tickets give the synchronous call's verdicts."""
import faulthandler
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_schnorr_comb as SC

pytestmark = pytest.mark.gpu
N = R.N
b32 = R.b32
NONE = 0xFFFFFFFF
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768
NSIG = 4096 + 37            # two ragged waves, no multiple of the finish kernel's group, more than one block of the sort
TIME_LIMIT = 180            # seconds per test: a hang ends the process, nothing else is started on the device


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


class thresholds_off:
    """the wave- and quad-per-signature ladders off (calls of this size would be delegated), defaults back afterwards"""

    def __init__(self, eng, mid=0):
        self.eng, self.mid = eng, mid

    def __enter__(self):
        self.eng.set_small_batch_max(0)
        self.eng.set_mid_batch_max(self.mid)

    def __exit__(self, *exc):
        self.eng.set_small_batch_max(ROW_DEFAULT)
        self.eng.set_mid_batch_max(QUAD_DEFAULT)


def _lifted(xs, odd_every=2):
    """X || Y rows for x-only keys that lift: every `odd_every`-th one stored with ODD y"""
    out = np.zeros((len(xs), 64), np.uint8)
    for j, x in enumerate(xs):
        pt = R.lift_x(int.from_bytes(bytes(x), "big"), 1 if j % odd_every == 1 else 0)
        out[j] = np.frombuffer(b32(pt[0]) + b32(pt[1]), np.uint8)
    return out


def _hits(ks, keys, pk):
    """signatures whose X the set holds as a valid key"""
    xs = {bytes(k[:32]) for k, v in zip(keys, ks.valid_keys()) if v}
    return sum(bytes(p) in xs for p in pk)


def _damage(rng, sig, msgs, idx):
    """a bit of r, of s or of the message (fixed-length rows, or a list of byte strings)"""
    for j, i in enumerate(idx):
        what, byte, bit = j % 3, int(rng.integers(0, 32)), 1 << int(rng.integers(0, 8))
        if what < 2:
            sig[i][32 * what + byte] ^= bit
        elif isinstance(msgs, list):
            m = bytearray(msgs[i] or b"x")
            m[byte % len(m)] ^= bit
            msgs[i] = bytes(m) if msgs[i] else b"x"
        else:
            msgs[i, byte] ^= bit


# ---- 1. fused verdicts ----
@pytest.fixture(scope="module")
def fused_cases(eng, oracle):
    """Two batches of 4096 + 37 signatures of 80 keys, a tenth damaged in r, s or the message.
    fixed: synth_schnorr_batch, 32-byte messages in an array; key 3 is in the set only off the curve (a miss that verifies),
    key 7 is X >= p in the batch and in the set, key 70 (outside the first 64) an X no point has.
    ragged: offset-delimited messages of every length around the SHA-256 block borders, zero included.
    Reference verdicts: the plain call under the same settings (thresholds off), checked against the oracle."""
    from secp256k1_voi_amd.synth import synth_schnorr_batch
    rng = np.random.default_rng(2001)
    cases = {}
    # fixed-length messages
    pk, msgs, sig = (np.array(a) for a in synth_schnorr_batch(eng, NSIG, 80, seed=2002))
    inv = np.arange(NSIG) % 80
    xs = pk[:80].copy()
    assert len({bytes(x) for x in xs}) == 80
    keys = _lifted(xs)
    keys[3, 63] ^= 1                                                                    # off the curve: X_3 still lifts
    not_x = next(x for x in range(2, 100) if R.lift_x(x, 0) is None)
    xs[7] = np.frombuffer(b32(R.P + 5), np.uint8)
    xs[70] = np.frombuffer(b32(not_x), np.uint8)
    keys[7, :32], keys[70, :32] = xs[7], xs[70]
    pk = np.ascontiguousarray(xs[inv])
    _damage(rng, sig, msgs, rng.permutation(NSIG)[:NSIG // 10])
    other = _lifted(np.array(synth_schnorr_batch(eng, 64, 64, seed=2003)[0]))
    cases["fixed"] = dict(pk=pk, msgs=msgs, sig=sig, keys=keys, other=other, misses=(3, 7, 70))
    # offset-delimited messages
    prng = random.Random(2004)
    d = [prng.randrange(1, N) for _ in range(80)]
    key = [i % 80 for i in range(NSIG)]
    rmsgs = [prng.randbytes(SC.MSG_LENGTHS[(i // 3) % len(SC.MSG_LENGTHS)]) for i in range(NSIG)]
    rpk, rsig, _ = SC.sign(eng, d, key, rmsgs, prng)
    rsig = [bytearray(s_) for s_ in rsig]
    assert any(len(m) == 0 for m in rmsgs)
    _damage(rng, rsig, rmsgs, rng.permutation(NSIG)[:NSIG // 10])
    rsig = [bytes(s_) for s_ in rsig]
    cases["ragged"] = dict(pk=np.frombuffer(b"".join(rpk), np.uint8).reshape(NSIG, 32).copy(), msgs=rmsgs,
                           sig=np.frombuffer(b"".join(rsig), np.uint8).reshape(NSIG, 64).copy(),
                           keys=_lifted([np.frombuffer(p_, np.uint8) for p_ in rpk[:80]], odd_every=3), other=other, misses=())
    with thresholds_off(eng):
        for name, c in cases.items():
            c["ref"] = eng.schnorr_verify_batch(c["pk"], c["msgs"], c["sig"])
            st = eng.key_grouping_stats()
            assert st["keyed"] + st["general"] == NSIG, (name, st)       # (not the wave- or quad-per-signature ladder)
            exp = SC.expected(oracle, c["pk"], c["msgs"] if isinstance(c["msgs"], list) else [bytes(m) for m in c["msgs"]], c["sig"])
            assert np.array_equal(c["ref"], exp), name
            assert 0.8 * NSIG < int(exp.sum()) < 0.92 * NSIG, (name, int(exp.sum()))
    f = cases["fixed"]
    under = lambda k: (np.arange(NSIG) % 80) == k
    assert f["ref"][under(3)].sum() > 40 and not f["ref"][under(7)].any() and not f["ref"][under(70)].any()
    return cases


LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_verdicts(eng, fused_cases, layout):
    import secp256k1_voi_amd as S
    sets = []
    with thresholds_off(eng):
        try:
            for name, c in fused_cases.items():
                pk, msgs, sig = c["pk"], c["msgs"], c["sig"]
                inv = np.arange(NSIG) % 80
                in_first = int(((inv < 64) & ~np.isin(inv, c["misses"])).sum())
                in_all = int((~np.isin(inv, c["misses"])).sum())
                for keys, hits in ((c["keys"][:64], in_first), (c["other"], 0), (c["keys"], in_all)):
                    ks = eng.keyset_create(keys, getattr(S, layout))
                    sets.append(ks)
                    assert ks.layout() == getattr(S, layout)
                    ks.index_create()
                    assert _hits(ks, keys, pk) == hits
                    got = eng.schnorr_verify_batch_bykey(ks, pk, msgs, sig)
                    st = eng.key_grouping_stats()
                    assert np.array_equal(got, c["ref"]), (name, len(keys), np.nonzero(got != c["ref"])[0][:10])
                    assert st["keyed"] == hits and st["general"] == NSIG - hits and st["tables"] == 0, (name, len(keys), st)
                    assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
        finally:
            for ks in sets:
                ks.close()


# ---- 2. the cases the lookup with key_bytes 32 in front of the by-index call gets wrong ----
@pytest.mark.parametrize("layout", ["KEYSET_JOINT5", "KEYSET_COMB"])
def test_invalid_entries_are_misses(eng, oracle, layout):
    """One set: A only as (X_A, Y_A ^ 1); B off the curve at index 0 and as the real point at index 4; C as -C only (odd Y);
    D twice; an entry with X >= p.  Valid signatures under A, B, C and D verify; A's count as misses, the others' as hits; a
    signature under X >= p is invalid.  The two-call route rejects A's."""
    import secp256k1_voi_amd as S
    rng = random.Random(2011)
    d = [rng.randrange(1, N) for _ in range(4)]
    key = [i % 4 for i in range(NSIG)]
    msgs = [rng.randbytes(32) for _ in range(NSIG)]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    big = b32(R.P + 5)
    is_big = np.array([i % 50 == 49 for i in range(NSIG)])
    pk = [big if is_big[i] else p_ for i, p_ in enumerate(pk)]
    A, B, C, D = (R.lift_x(int.from_bytes(pk[j], "big"), 0) for j in range(4))
    row = lambda x, y: np.frombuffer(b32(x) + b32(y), np.uint8)
    keys = np.stack([row(B[0], B[1] ^ 1), row(A[0], A[1] ^ 1), row(C[0], R.P - C[1]), row(D[0], D[1]), row(B[0], B[1]),
                     row(D[0], D[1]), row(R.P + 5, D[1])])
    assert keys[2, 63] & 1
    k = np.array(key)
    exp = SC.expected(oracle, pk, msgs, sig)
    assert exp[~is_big].all() and not exp[is_big].any()
    ks = eng.keyset_create(keys, getattr(S, layout))
    try:
        assert ks.valid_keys().tolist() == [0, 0, 1, 1, 1, 1, 0]
        ks.index_create()
        with thresholds_off(eng):
            got = eng.schnorr_verify_batch_bykey(ks, pk, msgs, sig)
            st = eng.key_grouping_stats()
            assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
            assert np.array_equal(got, eng.schnorr_verify_batch(pk, msgs, sig))
            for j in range(4):
                assert got[(k == j) & ~is_big].all(), "ABCD"[j]
            assert not got[is_big].any()
            misses = int(((k == 0) | is_big).sum())
            assert st["general"] == misses and st["keyed"] == NSIG - misses and st["tables"] == 0, st
            # the two-call route: the lowest index of ANY entry with this X, then the by-index call
            kidx = eng.keyset_lookup(ks, np.frombuffer(b"".join(pk), np.uint8).reshape(NSIG, 32), key_bytes=32)
            assert (kidx[(k == 0) & ~is_big] == 1).all() and (kidx[(k == 2) & ~is_big] == 2).all() and (kidx[(k == 3) & ~is_big] == 3).all()
            two = eng.schnorr_verify_batch_keyset(ks, kidx, msgs, sig)
            assert not two[(k == 0) & ~is_big].any(), "the two-call route rejects what the set lists only off the curve"
            assert two[(k >= 2) & ~is_big].all()
    finally:
        ks.close()


# ---- 3. exceptional lanes among hits and misses ----
def test_exceptional_lanes_among_hits_and_misses(eng, oracle):
    """1024 signatures over 16 keys, 8 of them in the set; per key every kind: 0 valid, 1 s = 0 (the generator part is the
    identity), 2 s = e d for an r that is an x coordinate (s G - e P is the identity), 3 signed with the nonce point's y odd,
    4 r >= p, 5 s >= n.  The plain call's and the oracle's verdicts; the lanes that end at infinity are the worklist's."""
    import secp256k1_voi_amd as S
    n, n_keys = 1024, 16
    rng = random.Random(2021)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    key = [i % n_keys for i in range(n)]
    kind = np.array([(i // n_keys) % 6 for i in range(n)])
    msgs = [rng.randbytes(SC.MSG_LENGTHS[i % len(SC.MSG_LENGTHS)]) for i in range(n)]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    _, sig_odd, _ = SC.sign(eng, d, key, msgs, rng, odd_nonce=True)
    for i in range(n):
        if kind[i] == 1:
            sig[i] = sig[i][:32] + bytes(32)
        elif kind[i] == 2:
            sig[i] = sig[i][:32] + b32(SC.challenge(sig[i][:32], pk[i], msgs[i]) * d_even[key[i]] % N)
        elif kind[i] == 3:
            sig[i] = sig_odd[i]
        elif kind[i] == 4:
            sig[i] = b32(R.P + i) + sig[i][32:]
        elif kind[i] == 5:
            sig[i] = sig[i][:32] + b32(min(N + i, 2**256 - 1) if i % 12 else 2**256 - 1)
    exp = SC.expected(oracle, pk, msgs, sig)
    assert exp[kind == 0].all() and not exp[kind != 0].any()
    in_set = np.array(key) < 8
    for side in (in_set, ~in_set):
        for kd in range(6):
            assert ((kind == kd) & side).sum() >= n // 16
    keys = _lifted([np.frombuffer(pk[j], np.uint8) for j in range(8)])
    sets = []
    with thresholds_off(eng):
        try:
            ref = eng.schnorr_verify_batch(pk, msgs, sig)
            assert np.array_equal(ref, exp)
            for layout in (S.KEYSET_COMB, S.KEYSET_JOINT5):
                ks = eng.keyset_create(keys, layout)
                sets.append(ks)
                ks.index_create()
                got = eng.schnorr_verify_batch_bykey(ks, pk, msgs, sig)
                st = eng.key_grouping_stats()
                assert np.array_equal(got, ref), np.nonzero(got != ref)[0][:10]
                assert st["keyed"] == int(in_set.sum()) and st["general"] == int((~in_set).sum()), st
                print("worklist lanes: %d (kinds 1 and 2: %d)" % (st["complete"], int(((kind == 1) | (kind == 2)).sum())))
                assert st["complete"] > 0
        finally:
            for ks in sets:
                ks.close()


# ---- 4. delegation and errors ----
def test_delegation_and_errors(eng):
    import torch
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_schnorr_batch
    pk, msgs, sig = (np.array(a) for a in synth_schnorr_batch(eng, 8192, 80, seed=2031))
    sig[::9, 40] ^= 2
    keys = _lifted(pk[:80])
    ks = eng.keyset_create(keys[:64], S.KEYSET_COMB)
    bare = eng.keyset_create(keys[:64], S.KEYSET_COMB)
    other_eng = S.Engine(0)
    try:
        ks.index_create()
        # default thresholds: calls of 1000 and of 8192 signatures ARE the plain call (no grouping, no worklist)
        for n in (1000, 8192):
            a = [np.ascontiguousarray(x[:n]) for x in (pk, msgs, sig)]
            got = eng.schnorr_verify_batch_bykey(ks, *a)
            st = eng.key_grouping_stats()
            assert np.array_equal(got, eng.schnorr_verify_batch(*a)) and 0 < int(got.sum()) < n
            assert st == dict(keyed=0, tables=0, general=0, complete=0), (n, st)
        n = 1000
        dev = torch.device("cuda", 0)
        t = [torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev) for x in (pk, msgs, sig)]
        out = torch.zeros(n, dtype=torch.uint8, device=dev)
        eng.schnorr_verify_batch_bykey_device(ks, n, t[0].data_ptr(), t[1].data_ptr(), 32, t[2].data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eng.schnorr_verify_batch(pk[:n], msgs[:n], sig[:n]))
        assert eng.key_grouping_stats() == dict(keyed=0, tables=0, general=0, complete=0)
        # n = 0
        assert eng.schnorr_verify_batch_bykey(ks, pk[:0], msgs[:0], sig[:0]).shape == (0,)
        assert eng.schnorr_verify_batch_bykey(ks, pk[:0], [], sig[:0]).shape == (0,)
        eng.schnorr_verify_batch_bykey_device(ks, 0, None, None, 0, None, None)
        # refusals
        a = [np.ascontiguousarray(x[:n]) for x in (pk, msgs, sig)]
        with pytest.raises(S.EngineError):
            eng.schnorr_verify_batch_bykey(bare, *a)                                   # no index: never built implicitly
        with pytest.raises(S.EngineError):
            eng.schnorr_verify_batch_bykey_submit(bare, *a)
        with pytest.raises(S.EngineError):
            eng.ecdsa_verify_batch_bykey_submit(bare, np.zeros((4, 64), np.uint8), *(np.zeros((4, 32), np.uint8),) * 3)
        with pytest.raises(S.EngineError):
            other_eng.schnorr_verify_batch_bykey(ks, *a)                               # a set of another engine
        with pytest.raises(S.EngineError):
            other_eng.schnorr_verify_batch_bykey_submit(ks, *a)
        for flags in (S.FORCE_COMPLETE, S.REJECT_MALLEABLE, S.FORCE_WORKLIST):
            with pytest.raises(S.EngineError):
                eng.schnorr_verify_batch_bykey_device(ks, n, t[0].data_ptr(), t[1].data_ptr(), 32, t[2].data_ptr(), out.data_ptr(), flags=flags)
        with pytest.raises(ValueError):
            eng.schnorr_verify_batch_bykey(ks, a[0], a[1], a[2][:-1])
        eng.wait_all()
    finally:
        other_eng.close()
        bare.close()
        ks.close()


# ---- 5. device form and tickets ----
def test_device_form_and_tickets(eng, fused_cases):
    import torch
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    c = fused_cases["fixed"]
    pk, msgs, sig = c["pk"], c["msgs"], c["sig"]
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, 80, seed=2041))
    s[::6, 11] ^= 8
    ekeys = np.unique(pub, axis=0)
    set_a = eng.keyset_create(np.concatenate([c["keys"][:64], ekeys[:40]]), S.KEYSET_JOINT5)
    set_b = eng.keyset_create(np.concatenate([ekeys, c["keys"]]), S.KEYSET_COMB)
    try:
        set_a.index_create()
        set_b.index_create()
        dev = torch.device("cuda", 0)
        with thresholds_off(eng):
            # the device form on a stream of the caller's, resident arrays
            stream = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(stream):
                t = [torch.from_numpy(x).to(dev) for x in (pk, msgs, sig)]
                out = torch.zeros(NSIG, dtype=torch.uint8, device=dev)
                eng.schnorr_verify_batch_bykey_device(set_a, NSIG, t[0].data_ptr(), t[1].data_ptr(), 32, t[2].data_ptr(), out.data_ptr(),
                                                      stream=stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(out.cpu().numpy(), c["ref"])
            st = eng.key_grouping_stats()
            assert st["keyed"] == _hits(set_a, np.concatenate([c["keys"][:64], ekeys[:40]]), pk) > 0 and st["keyed"] + st["general"] == NSIG
        # tickets: the batches of NSIG run the fused calls, the one of 1000 is delegated to the plain call inside its ticket
        with thresholds_off(eng, mid=1500):
            small = [np.ascontiguousarray(x[:1000]) for x in (pk, msgs, sig)]
            sync_s = {id(ks): eng.schnorr_verify_batch_bykey(ks, pk, msgs, sig) for ks in (set_a, set_b)}
            sync_e = {id(ks): eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s) for ks in (set_a, set_b)}
            assert eng.key_grouping_stats()["keyed"] == NSIG
            sync_small = eng.schnorr_verify_batch_bykey(set_a, *small)
            assert eng.key_grouping_stats() == dict(keyed=0, tables=0, general=0, complete=0)
            assert np.array_equal(sync_s[id(set_a)], c["ref"]) and np.array_equal(sync_s[id(set_b)], c["ref"])
            assert np.array_equal(sync_e[id(set_a)], eng.ecdsa_verify_batch(pub, dig, r, s)) and np.array_equal(sync_e[id(set_b)], sync_e[id(set_a)])
            assert np.array_equal(sync_small, c["ref"][:1000])
            tickets = []
            for j in range(4):
                ks = (set_a, set_b)[j & 1]
                if j == 2:
                    tickets.append((eng.schnorr_verify_batch_bykey_submit(ks, *small), sync_small))
                else:
                    tickets.append((eng.schnorr_verify_batch_bykey_submit(ks, pk, msgs if j else [bytes(m) for m in msgs], sig), sync_s[id(ks)]))
                tickets.append((eng.ecdsa_verify_batch_bykey_submit(ks, pub, dig, r, s), sync_e[id(ks)]))
            for j in (5, 2, 7, 0, 3, 6, 1, 4):                                         # out of order
                tk, want = tickets[j]
                assert np.array_equal(tk.wait(), want), j
            eng.wait_all()
    finally:
        set_a.close()
        set_b.close()
