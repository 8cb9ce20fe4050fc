"""k_verify_comb on the device (comb_ladder.hip): the comb ladder that needs no lead point - the top tooth's bit 18 set, the
first round one pair sum - against k_verify_fast<MODE_ECDSA_COMB> / <MODE_SCHNORR_COMB>, which S2K_COMB_LEAD=1 brings back
(read at every call).

Every case is one keyed call on comb tables run twice, knob unset and =1: the verdicts byte for byte the CPU oracle's both
times, the grouping statistics equal between the two.  Shapes: table counts on the edges of a wave and of a 256-lane block,
a seeded tenth damaged in r and in the digest, the chosen u2 of test_gpu_comb (the comb's corners, the lead's own bit among
them; u1 = 0 and R = the identity), one forced-worklist call; BIP-340 with x-only keys and over a comb key set that holds
odd-Y keys."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_comb as gc
import test_gpu_keyed as K
import test_gpu_schnorr_comb as SC

pytestmark = pytest.mark.gpu
N = R.N
KNOB = "S2K_COMB_LEAD"
COUNTS = (1, 8, 9, 33)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    assert KNOB not in os.environ and "S2K_KEYED_LADDER" not in os.environ and "S2K_KEY_TABLES_SPLIT" not in os.environ
    assert "COMB_LEAD=0" in S.load_library().s2k_build_config().decode()      # the default of this build: the new kernel
    e = S.Engine(0)
    e.set_small_batch_max(0)          # every batch here through the lane kernels: this file is about the comb ladder
    e.set_mid_batch_max(0)
    yield e
    e.close()


def _twice(monkeypatch, run):
    """run() with the knob unset and with =1; returns the two results"""
    out = []
    try:
        for lead in (False, True):
            if lead:
                monkeypatch.setenv(KNOB, "1")
            else:
                monkeypatch.delenv(KNOB, raising=False)
            out.append(run(lead))
    finally:
        monkeypatch.delenv(KNOB, raising=False)
    return out


def _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s, mode=None, flags=0, **grouping):
    """the ECDSA call on both kernels: the oracle's verdicts both times, equal statistics; returns them"""
    import secp256k1_voi_amd as S
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    eng.set_key_grouping(S.KEYS_ALWAYS if mode is None else mode, **grouping)
    eng.set_keyed_ladder(S.LADDER_COMB)

    def run(lead):
        got, st = K._device_run(eng, pub, dig, r, s, flags=flags)
        assert eng.last_keyed_ladder() == S.LADDER_COMB, "the call did not build comb tables"
        assert np.array_equal(got, exp), (lead, np.nonzero(got != exp)[0][:10])
        assert st["keyed"] + st["general"] == len(pub) and st["keyed"] > 0, (lead, st)
        return st
    try:
        stats = _twice(monkeypatch, run)
        assert stats[0] == stats[1]
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)
    return exp, stats[0]


def _damage_a_tenth(seed, r, dig):
    """a seeded tenth: half of it damaged in r, half in the digest; returns the indices"""
    n = len(r)
    rng = np.random.default_rng(seed)
    hit = rng.permutation(n)[:max(2, n // 10)]
    for arr, part in zip((r, dig), np.array_split(hit, 2)):
        arr[part, rng.integers(0, 32, size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    return hit


def _batch(eng, tables):
    """`tables` keys of 16 signatures; fewer than 256 signatures would not be grouped at all (KG_MIN_BATCH), so those cases
    are filled up to 256 with keys that sign once and run under KEYS_AUTO, as in test_gpu_finish_once"""
    fill = max(0, 256 - 16 * tables)
    pub, dig, r, s = K._ragged_batch(eng, 2000 + tables, np.array([16] * tables + [1] * fill))
    return fill, pub, dig, r, s


@pytest.mark.parametrize("tables", COUNTS)
def test_table_counts_with_a_damaged_tenth(eng, oracle, monkeypatch, tables):
    import secp256k1_voi_amd as S
    fill, pub, dig, r, s = _batch(eng, tables)
    hit = _damage_a_tenth(2100 + tables, r, dig)
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s, mode=S.KEYS_AUTO if fill else S.KEYS_ALWAYS)
    assert st["tables"] == tables and st["keyed"] == 16 * tables and st["general"] == fill
    keep = np.ones(len(pub), bool)
    keep[hit] = False
    assert exp[keep].all() and not exp[hit].any()


def test_forced_worklist(eng, oracle, monkeypatch):
    """S2K_ECDSA_FORCE_WORKLIST: every lane with a valid key leaves the new kernel through the worklist"""
    import secp256k1_voi_amd as S
    _, pub, dig, r, s = _batch(eng, 33)
    hit = _damage_a_tenth(2201, r, dig)
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s, flags=S.FORCE_WORKLIST)
    # (a damaged r can leave its range: such a lane is rejected by the preparation and is not queued)
    assert len(pub) - len(hit) <= st["complete"] <= len(pub) and 0 < exp.sum() == len(pub) - len(hit)


def test_chosen_scalars(eng, oracle, monkeypatch):
    """the chosen u2 of test_gpu_comb over nine keys: valid signatures with a random u1, u1 = 0 (the worklist's) and R = the
    identity (rejected).  2^133, (1 + lambda) 2^133 and the boundary halves are among them: the bit this ladder sets"""
    n_keys = 9
    rng = random.Random(2301)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    base = gc.chosen_u2()
    nsig = 3 * n_keys * len(base)
    u2 = [base[i % len(base)] for i in range(nsig)]
    key = [(i // len(base)) % n_keys for i in range(nsig)]
    kind = [i // (n_keys * len(base)) for i in range(nsig)]                          # 0 random u1, 1 u1 = 0, 2 R = identity
    u1 = [rng.randrange(N) if kd == 0 else 0 if kd == 1 else (-b * d[k]) % N for b, k, kd in zip(u2, key, kind)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    Rp = eng.scalar_base_mult_batch(gc._rows([v or 1 for v in kR]))
    Q = eng.scalar_base_mult_batch(gc._rows(d))[:, 1:]
    rr = [int.from_bytes(bytes(Rp[i, 1:33]), "big") % N if kR[i] else rng.randrange(1, N) for i in range(nsig)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    pub = np.ascontiguousarray(Q[key])
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, gc._rows(ee), gc._rows(rr), gc._rows(ss))
    assert st["keyed"] == nsig and st["tables"] == n_keys
    ok = np.array([kR[i] != 0 and rr[i] != 0 and ss[i] != 0 for i in range(nsig)])
    assert exp[ok].all() and not exp[~ok].any() and (~ok).sum() >= nsig // 3
    assert st["complete"] >= kind.count(1), "the u1 = 0 lanes are the worklist's"


# ==== BIP-340 ===============================================================================================================
def _schnorr_batch(eng, seed, tables):
    """`tables` x-only keys of 16 signatures (filled to 256 with keys that sign once), a seeded tenth damaged in r and in the
    message; returns pk, msgs, sig, the secret keys with even-y points, the key of every signature, and the fill"""
    fill = max(0, 256 - 16 * tables)
    sizes = [16] * tables + [1] * fill
    rng = random.Random(seed)
    key = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(sizes)), sizes)).tolist()
    d = [rng.randrange(1, N) for _ in sizes]
    msgs = [rng.randbytes(SC.MSG_LENGTHS[i % len(SC.MSG_LENGTHS)]) for i in range(len(key))]
    pk, sig, d_even = SC.sign(eng, d, key, msgs, rng)
    hit = np.random.default_rng(seed + 1).permutation(len(key))[:max(2, len(key) // 10)].tolist()
    for j, i in enumerate(hit):
        if j % 2:
            msgs[i] = msgs[i] + b"x"                                     # the digest
        else:
            b = bytearray(sig[i])
            b[rng.randrange(32)] ^= 1 << rng.randrange(8)                # r
            sig[i] = bytes(b)
    return pk, msgs, sig, d_even, key, fill, hit


@pytest.mark.parametrize("tables", COUNTS)
def test_schnorr_x_only_keys(eng, oracle, monkeypatch, tables):
    import secp256k1_voi_amd as S
    pk, msgs, sig, _, key, fill, hit = _schnorr_batch(eng, 2400 + tables, tables)
    exp = SC.expected(oracle, pk, msgs, sig)
    eng.set_key_grouping(S.KEYS_AUTO if fill else S.KEYS_ALWAYS)
    eng.set_keyed_ladder(S.LADDER_COMB)

    def run(lead):
        got = eng.schnorr_verify_batch(pk, msgs, sig)
        st = eng.key_grouping_stats()
        assert eng.last_keyed_ladder() == S.LADDER_COMB, "the call did not build comb tables"
        assert np.array_equal(got, exp), (lead, np.nonzero(got != exp)[0][:10])
        return st
    try:
        stats = _twice(monkeypatch, run)
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)
    assert stats[0] == stats[1]
    assert stats[0]["tables"] == tables and stats[0]["keyed"] == 16 * tables and stats[0]["general"] == fill
    keep = np.ones(len(key), bool)
    keep[hit] = False
    assert exp[keep].all() and not exp[hit].any()


def test_schnorr_comb_key_set_with_odd_y_keys(eng, oracle, monkeypatch):
    """a comb key set of 33 keys, every other one stored with ODD Y (both half scalars change sign in the ladder), 16
    signatures each, a tenth damaged"""
    import secp256k1_voi_amd as S
    nk = 33
    pk, msgs, sig, d_even, key, _, hit = _schnorr_batch(eng, 2501, nk)
    Pe = eng.scalar_base_mult_batch(SC._rows(d_even))                        # the even-y points
    keys = np.ascontiguousarray(Pe[:, 1:]).copy()
    for k in range(1, nk, 2):
        keys[k, 32:] = np.frombuffer(R.b32(R.P - int.from_bytes(bytes(Pe[k, 33:]), "big")), np.uint8)
    assert (keys[0:nk:2, 63] & 1).sum() == 0 and (keys[1:nk:2, 63] & 1).sum() == nk // 2
    exp = SC.expected(oracle, pk, msgs, sig)
    kidx = np.array(key, np.uint32)
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        def run(lead):
            got = eng.schnorr_verify_batch_keyset(ks, kidx, msgs, sig)
            assert np.array_equal(got, exp), (lead, np.nonzero(got != exp)[0][:10])
            return eng.key_grouping_stats()
        stats = _twice(monkeypatch, run)
    finally:
        ks.close()
    assert stats[0] == stats[1]
    keep = np.ones(len(key), bool)
    keep[hit] = False
    odd = np.array([k % 2 == 1 for k in key])
    assert exp[keep & odd].all() and exp[keep & ~odd].all() and not exp[hit].any()
