"""Key sets held as comb tables (S2K_KEYSET_COMB = 5: k_key_chain<false, KC_TEETH> and k_key_finish_comb_once on the set's own
buffer, 10 KiB per key; the ladders are k_verify_fast<MODE_ECDSA_COMB> and <MODE_SCHNORR_COMB> over the set's tables).

ECDSA and BIP-340 over such a set give the verdicts of the batch verifiers on the expanded keys and the CPU oracle's, byte for
byte: random and damaged signatures, keys that are no public keys, indices outside the set, chosen scalars at the comb's
corners, keys stored with odd Y under BIP-340, tickets of both kinds in flight together, one-key and duplicate-key sets, a group."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_comb as TC
import test_gpu_schnorr_comb as SC
from conftest import load_golden

pytestmark = pytest.mark.gpu
N = R.N
NSIG = 4096
b32 = R.b32


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def test_ecdsa_random_and_damaged(eng, oracle):
    """4096 signatures of 64 keys, a tenth damaged; two keys of the set are none; some indices point outside the set"""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, 64, seed=1801))
    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    keys, kidx = keys.copy(), inv.reshape(-1).astype(np.uint32)
    keys[3, 63] ^= 1                                                                    # off the curve
    keys[7, :32] = np.frombuffer(b32(R.P + 5), np.uint8)                                # x >= p: not canonical
    rng = np.random.default_rng(1802)
    hit = rng.permutation(NSIG)[:NSIG // 10]
    for arr, part in zip((r, s, dig), np.array_split(hit, 3)):
        arr[part, rng.integers(0, 32, size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    outside = rng.permutation(NSIG)[:40]
    kidx[outside] = len(keys) + (np.arange(40) % 3) * 1000
    kidx[outside[0]] = 0xFFFFFFFF
    inside = kidx < len(keys)
    full = np.zeros((NSIG, 64), np.uint8)
    full[inside] = keys[kidx[inside]]
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    chunks = eng.keyset_create(keys, S.KEYSET_CHUNKS)
    try:
        assert ks.layout() == S.KEYSET_COMB and len(ks) == 64
        valid = ks.valid_keys()
        assert not valid[3] and not valid[7] and valid.sum() == 62
        assert 64 * S.keyset_geometry(S.KEYSET_COMB)[2] <= ks.device_bytes() < chunks.device_bytes()
        got = eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r, s)
        st = eng.key_grouping_stats()
        assert np.array_equal(got, eng.ecdsa_verify_batch(full, dig, r, s))
        assert np.array_equal(got, oracle.ecdsa_verify_batch(full, dig, r, s, nthreads=os.cpu_count() or 1))
        assert np.array_equal(got, eng.ecdsa_verify_batch_keyset(chunks, kidx, dig, r, s))
        assert st["keyed"] == int(inside.sum()) and not got[~inside].any() and not got[(kidx == 3) | (kidx == 7)].any()
        assert 0.8 * NSIG < got.sum() < NSIG - NSIG // 10 + 1
        # the device form and the low-s rule over the same set
        assert np.array_equal(eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r, s, reject_malleable=True),
                              eng.ecdsa_verify_batch(full, dig, r, s, reject_malleable=True))
    finally:
        ks.close()
        chunks.close()


def test_ecdsa_chosen_scalars(eng, oracle):
    """test_gpu_comb.test_chosen_scalars over a 16-key comb set: u2 at the comb's corners with u1 random, u1 = 0 (the generator
    part is the identity: those lanes are the worklist's) and R = identity (rejected)"""
    import secp256k1_voi_amd as S
    n_keys = 16
    rng = random.Random(1811)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    base = TC.chosen_u2()
    u2 = [base[i % len(base)] for i in range(NSIG)]
    key = [(i // len(base)) % n_keys for i in range(NSIG)]
    kind = [0 if i < NSIG // 2 else 1 + (i & 1) for i in range(NSIG)]                # 0 random u1, 1 u1 = 0, 2 R = identity
    u1 = [rng.randrange(N) if kd == 0 else 0 if kd == 1 else (-b * d[k]) % N for b, k, kd in zip(u2, key, kind)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    Rp = eng.scalar_base_mult_batch(TC._rows([v or 1 for v in kR]))
    Q = np.ascontiguousarray(eng.scalar_base_mult_batch(TC._rows(d))[:, 1:])
    rr = [int.from_bytes(bytes(Rp[i, 1:33]), "big") % N if kR[i] else rng.randrange(1, N) for i in range(NSIG)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    dig, r, s = TC._rows(ee), TC._rows(rr), TC._rows(ss)
    exp = oracle.ecdsa_verify_batch(np.ascontiguousarray(Q[key]), dig, r, s, nthreads=os.cpu_count() or 1)
    ks = eng.keyset_create(Q, S.KEYSET_COMB)
    try:
        got = eng.ecdsa_verify_batch_keyset(ks, np.array(key, np.uint32), dig, r, s)
        st = eng.key_grouping_stats()
    finally:
        ks.close()
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    ok = np.array([kR[i] != 0 and rr[i] != 0 and ss[i] != 0 for i in range(NSIG)])
    assert exp[ok].all() and not exp[~ok].any() and (~ok).sum() >= NSIG // 4
    assert st["keyed"] == NSIG                                  # (a key-set call builds no tables: the statistics count none)
    assert st["complete"] >= int((np.array(kind) == 1).sum()), "the u1 = 0 lanes are the worklist's"


def test_schnorr_over_a_comb_set(eng, oracle):
    """BIP-340 verifies under lift_x(X): HALF of the set's keys are stored with odd Y (both half scalars change sign in the
    ladder).  Keys that are no points, indices outside the set, ragged messages, damaged signatures; the official vectors with
    their keys as the set; a BIP-340 ticket and an ECDSA ticket over comb sets in flight together."""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    rng = random.Random(1821)
    nk = 40
    d = [rng.randrange(1, N) for _ in range(nk)]
    key = [i % nk for i in range(NSIG)]
    msgs = [rng.randbytes(SC.MSG_LENGTHS[i % len(SC.MSG_LENGTHS)]) for i in range(NSIG)]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    P = eng.scalar_base_mult_batch(SC._rows(d_even))                         # the even-y points
    keys = np.zeros((nk + 2, 64), np.uint8)
    keys[:nk] = P[:, 1:]
    for k in range(1, nk, 2):                                               # every other key: the point with the OTHER y
        keys[k, 32:] = np.frombuffer(b32(R.P - int.from_bytes(bytes(P[k, 33:]), "big")), np.uint8)
    assert (keys[0:nk:2, 63] & 1).sum() == 0 and (keys[1:nk:2, 63] & 1).sum() == nk // 2
    keys[nk] = np.frombuffer(bytes(P[0, 1:33]) + b32((int.from_bytes(bytes(P[0, 33:]), "big") + 1) % R.P), np.uint8)   # not on the curve
    keys[nk + 1] = 0xFF                                                      # coordinates >= p
    kidx = list(key)
    for i in range(NSIG):
        kind = i % 7
        if kind == 1:
            sig[i] = sig[i][:32] + b32((int.from_bytes(sig[i][32:], "big") + 1) % N)
        elif kind == 2:
            msgs[i] = msgs[i] + b"x"
        elif kind == 3 and i % 21 == 3:
            sig[i] = b32(R.P + 5) + sig[i][32:]                              # r >= p
        elif kind == 4 and i % 28 == 4:
            kidx[i] = nk + (i % 2)                                           # a key of the set that is no public key
        elif kind == 5 and i % 35 == 5:
            kidx[i] = nk + 2 + (i % 3)                                       # an index outside the set
    pk = [bytes(keys[k][:32]) if k < nk + 2 else bytes(32) for k in kidx]
    out_of_set = np.array([k >= nk for k in kidx])
    exp = SC.expected(oracle, pk, msgs, sig)
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        assert ks.layout() == S.KEYSET_COMB and ks.valid_keys().tolist() == [1] * nk + [0, 0]
        got = eng.schnorr_verify_batch_keyset(ks, np.array(kidx, np.uint32), msgs, sig)
        assert not got[out_of_set].any()
        assert np.array_equal(got[~out_of_set], eng.schnorr_verify_batch(pk, msgs, sig)[~out_of_set])
        assert np.array_equal(got[~out_of_set], exp[~out_of_set])
        assert 0.5 * NSIG < int(got.sum()) < NSIG and got[0::14].all() and got[7::14].all()   # (untouched signatures under even-Y and odd-Y keys)
        # tickets of both kinds in flight together, each over a comb set
        pub, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, 32, seed=1822))
        s[::6, 11] ^= 8
        ekeys, einv = np.unique(pub, axis=0, return_inverse=True)
        eks = eng.keyset_create(ekeys, S.KEYSET_COMB)
        try:
            t1 = eng.schnorr_verify_batch_keyset_submit(ks, np.array(kidx, np.uint32), msgs, sig)
            t2 = eng.ecdsa_verify_batch_keyset_submit(eks, einv.reshape(-1).astype(np.uint32), dig, r, s)
            assert np.array_equal(t2.wait(), eng.ecdsa_verify_batch(pub, dig, r, s)) and np.array_equal(t1.wait(), got)
            eng.wait_all()
        finally:
            eks.close()
    finally:
        ks.close()
    # the official vectors: their x-only keys lifted (odd y for every other one); keys that do not lift stand in as off-curve points
    H = bytes.fromhex
    cases = load_golden("bip340.json")["cases"]
    vk = sorted({c["public_key"] for c in cases})
    vkeys = np.zeros((len(vk), 64), np.uint8)
    for j, hx in enumerate(vk):
        pt = R.lift_x(int(hx, 16), j % 2)                                    # (None: x >= p or no point has this x)
        vkeys[j] = np.frombuffer(H(hx) + (b32(pt[1]) if pt else bytes(32)), np.uint8)
    ks = eng.keyset_create(vkeys, S.KEYSET_COMB)
    try:
        vidx = np.array([vk.index(c["public_key"]) for c in cases], np.uint32)
        assert eng.schnorr_verify_batch_keyset(ks, vidx, [H(c["message"]) for c in cases], [H(c["signature"]) for c in cases]).tolist() == \
            [int(c["valid"]) for c in cases]
    finally:
        ks.close()


def test_small_and_duplicate_sets(eng, oracle):
    """A set of ONE key with 5000 signatures (every lane of every wave on the same table); a set that lists the same key three
    times; a set whose only key is no curve point; a call of one signature"""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    n = 5000
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, n, 1, seed=1831))
    s[::5, 9] ^= 0x20
    ref = eng.ecdsa_verify_batch(pub, dig, r, s)
    assert np.array_equal(ref[:512], oracle.ecdsa_verify_batch(pub[:512], dig[:512], r[:512], s[:512], nthreads=os.cpu_count() or 1))
    assert ref.sum() == n - len(range(0, n, 5))
    zeros = np.zeros(n, np.uint32)
    one = eng.keyset_create(pub[:1], S.KEYSET_COMB)
    try:
        assert one.layout() == S.KEYSET_COMB
        assert np.array_equal(eng.ecdsa_verify_batch_keyset(one, zeros, dig, r, s), ref)
        assert np.array_equal(eng.ecdsa_verify_batch_keyset(one, zeros[:1], dig[:1], r[:1], s[:1]), ref[:1])
        assert np.array_equal(eng.ecdsa_verify_batch_keyset(one, zeros[1:2], dig[1:2], r[1:2], s[1:2]), ref[1:2])
    finally:
        one.close()
    other = np.array(synth_batch(eng, 1, 1, seed=1832)[0])
    dup = eng.keyset_create(np.concatenate([pub[:1], other, pub[:1], pub[:1]]), S.KEYSET_COMB)       # copies of the key at 0, 2, 3
    try:
        kidx = np.array([(0, 2, 3, 1)[i % 4] for i in range(n)], np.uint32)
        got = eng.ecdsa_verify_batch_keyset(dup, kidx, dig, r, s)
        assert np.array_equal(got[kidx != 1], ref[kidx != 1]) and not got[kidx == 1].any()
    finally:
        dup.close()
    bad = pub[:1].copy()
    bad[0, 63] ^= 1
    nokey = eng.keyset_create(bad, S.KEYSET_COMB)
    try:
        assert not nokey.valid_keys().any() and not eng.ecdsa_verify_batch_keyset(nokey, zeros, dig, r, s).any()
    finally:
        nokey.close()


def test_group_keyset_two_members_one_device(eng, oracle):
    """Group.keyset_create(keys, KEYSET_COMB): the comb set on both members (two contexts on device 0), batches sharded across
    them; the single-context verdicts - ragged sizes, a size below the member count, an empty batch, two batches in flight"""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    nk, total = 100, 6000
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, total, nk, seed=1841))
    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    keys, kidx = keys.copy(), inv.reshape(-1).astype(np.uint32)
    keys[9, 1] ^= 0x10                                                 # no public key
    rng = np.random.default_rng(1842)
    for i in range(0, total, 8):
        a = (dig, r, s)[int(rng.integers(0, 3))]
        a[i, int(rng.integers(0, 32))] ^= 1 << int(rng.integers(0, 8))
    kidx[5] = len(keys)
    inside = kidx < len(keys)
    full = np.zeros((total, 64), np.uint8)
    full[inside] = keys[kidx[inside]]
    ks1 = eng.keyset_create(keys, S.KEYSET_COMB)
    g = S.Group([0, 0])
    try:
        ref = eng.ecdsa_verify_batch_keyset(ks1, kidx, dig, r, s)
        assert np.array_equal(ref, oracle.ecdsa_verify_batch(full, dig, r, s, nthreads=os.cpu_count() or 1))
        assert 0 < int(ref.sum()) < total and not ref[5] and not ref[kidx == 9].any()
        gks = g.keyset_create(keys, S.KEYSET_COMB)
        try:
            assert len(gks) == len(keys) and gks.layout() == S.KEYSET_COMB and gks.device_bytes() == ks1.device_bytes()
            for lo, n in ((0, total), (7, 4097), (11, 1), (0, 0), (300, 513)):
                got = g.ecdsa_verify_batch_keyset(gks, kidx[lo:lo + n], dig[lo:lo + n], r[lo:lo + n], s[lo:lo + n])
                assert np.array_equal(got, ref[lo:lo + n]), (lo, n)
            cuts = [(0, 3000), (3000, 3000)]
            tickets = [g.ecdsa_verify_batch_keyset_submit(gks, kidx[a:a + n], dig[a:a + n], r[a:a + n], s[a:a + n]) for a, n in cuts]
            for t, (a, n) in zip(tickets, cuts):
                assert np.array_equal(t.wait(), ref[a:a + n])
        finally:
            gks.close()
    finally:
        g.close()
        ks1.close()
