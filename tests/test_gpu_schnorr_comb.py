"""BIP-340 per-signature verification on comb tables (keyed.hip: k_key_chain<true, KC_TEETH> - x-only keys validated and lifted,
then the comb's chain -, k_key_finish_comb_once; verify_fast.h: k_verify_fast<MODE_SCHNORR_COMB>): what s2k_schnorr_verify_batch
builds for its repeated keys by default.

Every case is one call of 4096 signatures (the padded official vectors: 266) with the grouping set by name (KEYS_ALWAYS /
KEYS_AUTO: calls this small would otherwise take the wave- or quad-per-signature ladders), run on LADDER_COMB and on
LADDER_WINDOW: the verdicts byte for byte against the CPU oracle's schnorr_verify, s2k_ctx_last_keyed_ladder says which tables
ran, and the grouping statistics of the two ladders agree except for `complete`."""
import hashlib
import os
import random

import numpy as np
import pytest

import pyref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
N = R.N
NSIG = 4096
TAG = hashlib.sha256(b"BIP0340/challenge").digest()
MSG_LENGTHS = (0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 200)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    assert "S2K_KEYED_LADDER" not in os.environ and "S2K_KEY_TABLES_SPLIT" not in os.environ
    e = S.Engine(0)
    yield e
    e.close()


def _rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), np.uint8).reshape(-1, 32).copy()


def challenge(rx, px, m):
    return int.from_bytes(hashlib.sha256(TAG + TAG + rx + px + m).digest(), "big") % N


def sign(eng, d, key, msgs, rng, odd_nonce=False):
    """BIP-340 signatures of msgs[i] under key d[key[i]] (schnorr.go:158-218: even-y key and nonce points, e = tagged hash,
    s = k + e d), the point multiplications on the engine.  odd_nonce: the nonce point with ODD y is kept instead - the
    signature (x(R), s) then verifies to -R' = the point with the right x and the wrong y.
    Returns (x-only keys per signature as a list of bytes, signatures as a list of bytes, the even-y secret keys)."""
    P = eng.scalar_base_mult_batch(_rows(d))
    d = [N - x if P[j, 64] & 1 else x for j, x in enumerate(d)]
    k = [rng.randrange(1, N) for _ in msgs]
    Rp = eng.scalar_base_mult_batch(_rows(k))
    k = [N - x if bool(Rp[i, 64] & 1) != odd_nonce else x for i, x in enumerate(k)]
    pk, sig = [], []
    for i, m in enumerate(msgs):
        rx, px = bytes(Rp[i, 1:33]), bytes(P[key[i], 1:33])
        pk.append(px)
        sig.append(rx + R.b32((k[i] + challenge(rx, px, m) * d[key[i]]) % N))
    return pk, sig, d


def expected(oracle, pk, msgs, sig):
    return np.array([1 if oracle.schnorr_verify(bytes(p_), bytes(m_), bytes(s_)) == 1 else 0 for p_, m_, s_ in zip(pk, msgs, sig)], np.uint8)


def both_ladders(eng, pk, msgs, sig, exp, mode=None, **grouping):
    """the call on comb tables and on window tables: `exp` both times; returns the comb run's statistics"""
    import secp256k1_voi_amd as S
    eng.set_key_grouping(S.KEYS_ALWAYS if mode is None else mode, **grouping)
    stats = {}
    try:
        for ladder in (S.LADDER_COMB, S.LADDER_WINDOW):
            eng.set_keyed_ladder(ladder)
            got = eng.schnorr_verify_batch(pk, msgs, sig)
            assert eng.last_keyed_ladder() == ladder, "the call did not build the tables that were asked for"
            st = eng.key_grouping_stats()
            assert np.array_equal(got, exp), (ladder, np.nonzero(got != exp)[0][:10])
            assert st["keyed"] + st["general"] == len(exp) and st["keyed"] > 0, (ladder, st)
            stats[ladder] = st
        assert {k: v for k, v in stats[S.LADDER_COMB].items() if k != "complete"} == \
               {k: v for k, v in stats[S.LADDER_WINDOW].items() if k != "complete"}
    finally:
        eng.set_keyed_ladder(S.LADDER_COMB)
        eng.set_key_grouping(S.KEYS_AUTO)
    return stats[S.LADDER_COMB]


MIXED_SIZES = np.array([64] * 40 + [16] * 60 + [5] * 40 + [4] * 50 + [3] * 40 + [1] * 56)


@pytest.fixture(scope="module")
def mixed(eng, oracle):
    """keys with 1, 3, 4, 5, 16 and 64 signatures, messages of every length around the SHA-256 block borders, a group under an x
    that no point has and one under x >= p, a seeded tenth damaged in r, s or the message, some r >= p and some s >= n"""
    assert MIXED_SIZES.sum() == NSIG
    rng = random.Random(1701)
    key = np.random.default_rng(1702).permutation(np.repeat(np.arange(len(MIXED_SIZES)), MIXED_SIZES)).tolist()
    d = [rng.randrange(1, N) for _ in MIXED_SIZES]
    msgs = [rng.randbytes(MSG_LENGTHS[i % len(MSG_LENGTHS)]) for i in range(NSIG)]
    pk, sig, _ = sign(eng, d, key, msgs, rng)
    k16, k5 = (int(np.nonzero(MIXED_SIZES == c)[0][0]) for c in (16, 5))
    not_x = next(x for x in range(2, 100) if R.lift_x(x, 0) is None)
    bad = {k16: R.b32(not_x), k5: R.b32(R.P + 5)}
    pk = [bad.get(key[i], p_) for i, p_ in enumerate(pk)]
    hit = np.random.default_rng(1703).permutation(NSIG)[:NSIG // 10].tolist()
    for j, i in enumerate(hit):
        what, byte, bit = j % 3, rng.randrange(32), 1 << rng.randrange(8)
        if what == 2 and msgs[i]:
            m = bytearray(msgs[i])
            m[byte % len(m)] ^= bit
            msgs[i] = bytes(m)
        elif what == 2:
            msgs[i] = b"x"
        else:
            s_ = bytearray(sig[i])
            s_[32 * what + byte] ^= bit
            sig[i] = bytes(s_)
    hit_set = set(hit)
    rest = [i for i in range(NSIG) if i not in hit_set]
    for j, i in enumerate(rest[:24]):
        sig[i] = (R.b32(R.P + j) + sig[i][32:]) if j % 2 else (sig[i][:32] + R.b32(min(N + j // 2, 2**256 - 1) if j % 4 else 2**256 - 1))
    exp = expected(oracle, pk, msgs, sig)
    under_bad = np.array([key[i] in bad for i in range(NSIG)])
    assert not exp[under_bad].any() and not exp[rest[:24]].any() and not exp[hit].any()
    assert exp.sum() == NSIG - NSIG // 10 - 24 - int(under_bad[rest[24:]].sum())
    return pk, msgs, sig, exp


def test_mixed_batch(eng, mixed):
    import secp256k1_voi_amd as S
    pk, msgs, sig, exp = mixed
    assert len({len(m) for m in msgs}) >= len(MSG_LENGTHS)
    st = both_ladders(eng, pk, msgs, sig, exp)
    assert st["keyed"] == NSIG and st["tables"] == len(MIXED_SIZES) == len(set(pk))
    # the default threshold: groups of at least four on the tables, the rest on the general ladder (MODE_SCHNORR_LEFT)
    st4 = both_ladders(eng, pk, msgs, sig, exp, mode=S.KEYS_AUTO)
    assert st4["keyed"] == int(MIXED_SIZES[MIXED_SIZES >= 4].sum()) and st4["general"] == int(MIXED_SIZES[MIXED_SIZES < 4].sum())
    assert st4["tables"] == int((MIXED_SIZES >= 4).sum())


def test_minus_r_family_and_ladders_that_end_at_infinity(eng, oracle):
    """Four kinds, 64 keys with 64 signatures each.  0: signed with the nonce point's y ODD - s G - e P is the point with
    x = r and odd y, finite, rejected by the even-y rule of k_affine_finish.  1: a valid signature's (x(R), n - s): rejected.
    2: valid (the control).  3: s = e d for an r that is an x coordinate - s G - e P is the identity: the ladder's last
    addition meets opposite points, Z = 0 is what it leaves, and the lane is the worklist kernel's, which rejects it.
    (Kinds 0 and 1 end on finite points, so only kind 3 is counted on the worklist.)"""
    rng = random.Random(1711)
    n_keys = 64
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    key = [i % n_keys for i in range(NSIG)]
    kind = [(i // n_keys) % 4 for i in range(NSIG)]
    msgs = [rng.randbytes(MSG_LENGTHS[i % len(MSG_LENGTHS)]) for i in range(NSIG)]
    pk, sig, d_even = sign(eng, d, key, msgs, rng)
    _, sig_odd, _ = sign(eng, d, key, msgs, rng, odd_nonce=True)
    for i in range(NSIG):
        if kind[i] == 0:
            sig[i] = sig_odd[i]
        elif kind[i] == 1:
            sig[i] = sig[i][:32] + R.b32(N - int.from_bytes(sig[i][32:], "big"))
        elif kind[i] == 3:
            sig[i] = sig[i][:32] + R.b32(challenge(sig[i][:32], pk[i], msgs[i]) * d_even[key[i]] % N)
    exp = expected(oracle, pk, msgs, sig)
    kind = np.array(kind)
    assert exp[kind == 2].all() and not exp[kind != 2].any()
    for i in np.nonzero(kind == 0)[0][:8]:                       # what kind 0 is: the right x under the wrong y
        e = challenge(sig[i][:32], pk[i], msgs[i])
        Rv = R.add(R.mul(int.from_bytes(sig[i][32:], "big"), R.G), R.neg(R.mul(e, R.lift_x(int.from_bytes(pk[i], "big"), 0))))
        assert R.b32(Rv[0]) == sig[i][:32] and Rv[1] & 1
    st = both_ladders(eng, pk, msgs, sig, exp)
    assert st["keyed"] == NSIG and st["tables"] == n_keys
    print("worklist lanes: %d (kind 3: %d)" % (st["complete"], int((kind == 3).sum())))
    assert st["complete"] >= int((kind == 3).sum()), "the ladders that end at infinity are the worklist's"


def test_official_vectors_padded_to_a_grouped_call(eng, oracle):
    import secp256k1_voi_amd as S
    cases = load_golden("bip340.json")["cases"]
    reps = -(-256 // len(cases))
    items = [c for _ in range(reps) for c in cases]
    assert len(items) >= 256
    H = bytes.fromhex
    pk, msgs, sig = [H(c["public_key"]) for c in items], [H(c["message"]) for c in items], [H(c["signature"]) for c in items]
    exp = np.array([int(c["valid"]) for c in items], np.uint8)
    assert np.array_equal(exp, expected(oracle, pk, msgs, sig)) and 0 < exp.sum() < len(exp)
    st = both_ladders(eng, pk, msgs, sig, exp)
    assert st["keyed"] == len(items) and st["tables"] == len(set(pk))


def test_table_cap_sends_groups_to_the_general_ladder(eng, oracle):
    """a cap of 32 tables for 4096 signatures raises the threshold to 128 per key: the sixteen keys that have them get
    tables, the groups of 64 and 16 take the general ladder over the rest list"""
    sizes = np.array([128] * 16 + [64] * 16 + [16] * 64)
    assert sizes.sum() == NSIG
    rng = random.Random(1731)
    key = np.random.default_rng(1732).permutation(np.repeat(np.arange(len(sizes)), sizes)).tolist()
    msgs = [rng.randbytes(32) for _ in range(NSIG)]
    pk, sig, _ = sign(eng, [rng.randrange(1, N) for _ in sizes], key, msgs, rng)
    for i in range(0, NSIG, 11):
        sig[i] = sig[i][:41] + bytes([sig[i][41] ^ 4]) + sig[i][42:]
    exp = expected(oracle, pk, msgs, sig)
    assert exp.sum() == NSIG - len(range(0, NSIG, 11))
    st = both_ladders(eng, pk, np.frombuffer(b"".join(msgs), np.uint8).reshape(NSIG, 32), sig, exp, max_tables=32)
    assert st["tables"] == 16 and st["keyed"] == 2048 and st["general"] == 2048


def test_window_path_by_environment_and_split_knob(mixed):
    """S2K_KEYED_LADDER=window at context creation, and S2K_KEY_TABLES_SPLIT at any call, select the window tables for a
    BIP-340 call as they do for an ECDSA one; without grouping no tables are built"""
    import secp256k1_voi_amd as S
    pk, msgs, sig, exp = mixed
    os.environ["S2K_KEYED_LADDER"] = "window"
    try:
        e2 = S.Engine(0)
    finally:
        del os.environ["S2K_KEYED_LADDER"]
    try:
        e2.set_key_grouping(S.KEYS_ALWAYS)
        assert np.array_equal(e2.schnorr_verify_batch(pk, msgs, sig), exp) and e2.last_keyed_ladder() == S.LADDER_WINDOW
        e2.set_keyed_ladder(S.LADDER_COMB)
        assert np.array_equal(e2.schnorr_verify_batch(pk, msgs, sig), exp) and e2.last_keyed_ladder() == S.LADDER_COMB
        os.environ["S2K_KEY_TABLES_SPLIT"] = "1"
        try:
            got = e2.schnorr_verify_batch(pk, msgs, sig)
        finally:
            del os.environ["S2K_KEY_TABLES_SPLIT"]
        assert np.array_equal(got, exp) and e2.last_keyed_ladder() == S.LADDER_WINDOW
        e2.set_key_grouping(S.KEYS_OFF)
        assert np.array_equal(e2.schnorr_verify_batch(pk, msgs, sig), exp) and e2.last_keyed_ladder() == -1
    finally:
        e2.close()
