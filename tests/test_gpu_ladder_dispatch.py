"""Every ladder launch_ladder (lane_kernels.hip) can choose, at the smallest shape that can still go wrong: 257 signatures - one
full workgroup of k_verify_fast and one lane -, 250 of them under three keys (one stored with odd Y) and 7 under keys that
occur once, every fourth one damaged.  The wave- and quad-per-signature ladders are switched off, so each call runs the lane
kernels: the plain modes (ECDSA, BIP-340, recovery, the point entry), the keyed / comb / "left" modes of the grouped flows
under both ladder settings, and the five key-set layouts for ECDSA and BIP-340.  A wrong row in the switch over MODE_* would
otherwise show only in whichever older test happens to use that layout.

Expected values come from the CPU oracle alone; every case compares the whole output array."""
import random

import numpy as np
import pytest

import pyref as R

pytestmark = pytest.mark.gpu
N, P = R.N, R.P
b32 = R.b32
NSIG, SHARED, NKEYS = 257, 250, 10        # signatures; those under the three shared keys; keys in all


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    e.set_small_batch_max(0)
    e.set_mid_batch_max(0)
    e.set_keyset_small_batch_max(0)
    yield e
    e.close()


def _rows(vals):
    return np.frombuffer(b"".join(vals), np.uint8).reshape(len(vals), -1).copy()


def make_batch(oracle):
    """The keys, who signs what, ECDSA signatures with their recovery ids and BIP-340 signatures, damaged every fourth; the
    oracle's answers to all of them."""
    rng = random.Random(1501)
    d, pts = [], []
    while len(d) < NKEYS:                  # key 0: even Y, key 1: odd Y, the rest as they come
        x = rng.randrange(1, N)
        q = oracle.scalar_base_mult_vartime(b32(x))
        if len(d) < 2 and (q[64] & 1) != len(d):
            continue
        d.append(x)
        pts.append(q)
    keys = _rows([q[1:] for q in pts])
    assert keys[0, 63] & 1 == 0 and keys[1, 63] & 1 == 1
    key = [i % 3 for i in range(SHARED)] + list(range(3, NKEYS))
    rng.shuffle(key)
    key = np.array(key, np.uint32)
    # ---- ECDSA, recoverable
    dig, rr, ss, rid = [], [], [], []
    for i in range(NSIG):
        digest, k = rng.randbytes(32), rng.randrange(1, N)
        Rp = oracle.scalar_base_mult_vartime(b32(k))
        x, r = int.from_bytes(Rp[1:33], "big"), int.from_bytes(Rp[1:33], "big") % N
        s = pow(k, -1, N) * (int.from_bytes(digest, "big") + r * d[key[i]]) % N
        v = (Rp[64] & 1) | (2 if x >= N else 0)
        if s > N // 2:
            s, v = N - s, v ^ 1
        if i % 4 == 0:                     # damaged: r, s, the digest, r = 0, s = 0, r not canonical, an id that does not exist
            kind = (i // 4) % 7
            if kind == 0: r = (r ^ (1 << rng.randrange(250))) % N or 1
            elif kind == 1: s = (s + 1 + rng.randrange(1000)) % N or 1
            elif kind == 2: digest = bytes([digest[0] ^ 0x40]) + digest[1:]
            elif kind == 3: r = 0
            elif kind == 4: s = 0
            elif kind == 5: r = N + r % 1000
            else: v = 4 + (i & 3)
        dig.append(digest), rr.append(b32(r)), ss.append(b32(s)), rid.append(v)
    dig, rr, ss, rid = _rows(dig), _rows(rr), _rows(ss), np.array(rid, np.uint8)
    pub = np.ascontiguousarray(keys[key])
    # ---- BIP-340 (signed under the even-Y point of the key, verified under its X)
    msgs, sig = [], []
    for i in range(NSIG):
        m, k0 = rng.randbytes(32), rng.randrange(1, N)
        dd = d[key[i]] if keys[key[i], 63] & 1 == 0 else N - d[key[i]]
        Rp = oracle.scalar_base_mult_vartime(b32(k0))
        k = N - k0 if Rp[64] & 1 else k0
        e = int.from_bytes(R.tagged_hash("BIP0340/challenge", Rp[1:33], bytes(keys[key[i], :32]), m), "big") % N
        rb, s = Rp[1:33], (k + e * dd) % N
        if i % 4 == 0:                     # damaged: s, the message, r >= p, another r, s >= n
            kind = (i // 4) % 5
            if kind == 0: s = (s + 1) % N
            elif kind == 1: m = bytes([m[0] ^ 1]) + m[1:]
            elif kind == 2: rb = b32(P + 5)
            elif kind == 3: rb = b32((int.from_bytes(rb, "big") + 1) % P)
            else: s = N + s % 1000
        msgs.append(m), sig.append(rb + b32(s))
    msgs, sig = _rows(msgs), _rows(sig)
    pk32 = np.ascontiguousarray(pub[:, :32])
    # ---- the point entry: u1 G + u2 P, every fourth one the identity (u1 = -u2 d)
    u1, u2 = [], []
    for i in range(NSIG):
        b = rng.randrange(1, N)
        u2.append(b32(b))
        u1.append(b32((-b * d[key[i]]) % N if i % 4 == 0 else rng.randrange(N)))
    pts65 = _rows([pts[k] for k in key])
    exp_ecdsa = oracle.ecdsa_verify_batch(pub, dig, rr, ss)
    exp_schnorr = np.array([1 if oracle.schnorr_verify(bytes(pk32[i]), bytes(msgs[i]), bytes(sig[i])) else 0 for i in range(NSIG)], np.uint8)
    rec = [oracle.ecdsa_recover(bytes(dig[i]), bytes(rr[i]), bytes(ss[i]), int(rid[i])) for i in range(NSIG)]
    exp_rec_ok = np.array([q is not None for q in rec], np.uint8)
    exp_rec = _rows([q if q is not None else bytes(65) for q in rec])
    exp_pts = _rows([oracle.double_scalar_mult_basepoint_vartime(u1[i], u2[i], bytes(pts65[i])) for i in range(NSIG)])
    for e in (exp_ecdsa, exp_schnorr, exp_rec_ok):
        assert 0 < int(e.sum()) < NSIG, "accepted and rejected signatures"
    both = (exp_ecdsa == 1) & (exp_rec_ok == 1)              # (the recovery ids above are the right ones)
    assert both.sum() > NSIG // 2 and np.array_equal(exp_rec[both, 1:], pub[both])
    zero = ~exp_pts.any(axis=1)
    assert zero[::4].all() and not zero[1::4].any()
    return dict(keys=keys, key=key, pub=pub, dig=dig, r=rr, s=ss, rid=rid, pk32=pk32, msgs=msgs, sig=sig, u1=_rows(u1), u2=_rows(u2), pts65=pts65,
                exp_ecdsa=exp_ecdsa, exp_schnorr=exp_schnorr, exp_rec=exp_rec, exp_rec_ok=exp_rec_ok, exp_pts=exp_pts)


@pytest.fixture(scope="module")
def batch(oracle):
    return make_batch(oracle)


def test_plain_ecdsa(eng, batch):
    """grouping off: MODE_ECDSA"""
    import secp256k1_voi_amd as S
    eng.set_key_grouping(S.KEYS_OFF)
    try:
        got = eng.ecdsa_verify_batch(batch["pub"], batch["dig"], batch["r"], batch["s"])
        st = eng.key_grouping_stats()
    finally:
        eng.set_key_grouping(S.KEYS_ADAPTIVE)
    assert np.array_equal(got, batch["exp_ecdsa"]), np.nonzero(got != batch["exp_ecdsa"])[0][:10]
    assert st["keyed"] == 0 and eng.last_keyed_ladder() == -1


def test_plain_schnorr(eng, batch):
    """grouping off: MODE_SCHNORR"""
    import secp256k1_voi_amd as S
    eng.set_key_grouping(S.KEYS_OFF)
    try:
        got = eng.schnorr_verify_batch(batch["pk32"], batch["msgs"], batch["sig"])
        st = eng.key_grouping_stats()
    finally:
        eng.set_key_grouping(S.KEYS_ADAPTIVE)
    assert np.array_equal(got, batch["exp_schnorr"]), np.nonzero(got != batch["exp_schnorr"])[0][:10]
    assert st["keyed"] == 0 and eng.last_keyed_ladder() == -1
    assert 0 < int(got.sum()) < NSIG


@pytest.mark.parametrize("ladder", ["comb", "window"])
@pytest.mark.parametrize("algo", ["ecdsa", "schnorr"])
def test_grouped(eng, batch, algo, ladder):
    """S2K_KEYS_ALWAYS under both s2k_ctx_set_keyed_ladder settings: MODE_*_COMB or MODE_*_KEYED for the three shared keys and
    MODE_*_LEFT for the rest.  (max_tables = 64: 257 signatures on at most 64 tables raise the call's threshold to five per
    key - keyed.hip: key_group_plan -, so the seven keys that occur once take the general ladder.)"""
    import secp256k1_voi_amd as S
    want = S.LADDER_COMB if ladder == "comb" else S.LADDER_WINDOW
    eng.set_key_grouping(S.KEYS_ALWAYS, max_tables=64)
    eng.set_keyed_ladder(want)
    try:
        if algo == "ecdsa":
            got, exp = eng.ecdsa_verify_batch(batch["pub"], batch["dig"], batch["r"], batch["s"]), batch["exp_ecdsa"]
        else:
            got, exp = eng.schnorr_verify_batch(batch["pk32"], batch["msgs"], batch["sig"]), batch["exp_schnorr"]
        st, last = eng.key_grouping_stats(), eng.last_keyed_ladder()
    finally:
        eng.set_keyed_ladder(S.LADDER_COMB)
        eng.set_key_grouping(S.KEYS_ADAPTIVE)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    assert last == want
    assert st["keyed"] == SHARED and st["general"] == NSIG - SHARED and st["tables"] == 3, st


def test_recovery(eng, batch):
    """MODE_RECOVER"""
    pub65, ok = eng.ecdsa_recover_batch(batch["dig"], batch["r"], batch["s"], batch["rid"])
    assert np.array_equal(ok, batch["exp_rec_ok"]), np.nonzero(ok != batch["exp_rec_ok"])[0][:10]
    assert np.array_equal(pub65, batch["exp_rec"])


def test_point_entry(eng, batch):
    """MODE_POINT: u1 G + u2 P through the verification ladder; every fourth result is the identity"""
    import secp256k1_voi_amd as S
    got = eng.double_scalar_mult_basepoint_batch_ex(S.IMPL_FAST, batch["u1"], batch["u2"], batch["pts65"])
    assert np.array_equal(got, batch["exp_pts"]), np.nonzero((got != batch["exp_pts"]).any(axis=1))[0][:10]


LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("algo", ["ecdsa", "schnorr"])
def test_keyset(eng, batch, algo, layout):
    """every layout the header defines, for ECDSA (MODE_ECDSA_KEYSET*, MODE_ECDSA_COMB) and BIP-340 (the mode + 4,
    MODE_SCHNORR_COMB); one signature names a key outside the set and stays invalid"""
    import secp256k1_voi_amd as S
    kidx = batch["key"].copy()
    out = 9                                                    # (a signature that is valid under its own key)
    assert batch["exp_ecdsa"][out] and batch["exp_schnorr"][out]
    kidx[out] = NKEYS + 3
    ks = eng.keyset_create(batch["keys"], getattr(S, layout))
    try:
        assert ks.layout() == getattr(S, layout)
        if algo == "ecdsa":
            got, exp = eng.ecdsa_verify_batch_keyset(ks, kidx, batch["dig"], batch["r"], batch["s"]), batch["exp_ecdsa"].copy()
        else:
            got, exp = eng.schnorr_verify_batch_keyset(ks, kidx, batch["msgs"], batch["sig"]), batch["exp_schnorr"].copy()
        last = eng.last_keyset_ladder()
    finally:
        ks.close()
    exp[out] = 0
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    assert last == S.KEYSET_LADDER_LANE
    assert 0 < int(got.sum()) < NSIG
