"""The comb tables and their ladder on the device (keyed.hip: k_key_chain on the comb's geometry with kc_sets, k_key_finish_comb; verify_fast.h:
k_verify_fast<MODE_ECDSA_COMB>): what an ECDSA verification call builds for its repeated keys by default.

Every case is one call of 4096 signatures with the grouping set by name (KEYS_ALWAYS / KEYS_AUTO: calls this small
would otherwise take the wave- or quad-per-signature ladders), its verdicts byte for byte against the CPU oracle and
against the same call on the window path (set_keyed_ladder), and s2k_ctx_last_keyed_ladder says which tables ran."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_keyed as K

pytestmark = pytest.mark.gpu
N = R.N
NSIG = 4096


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    assert "S2K_KEYED_LADDER" not in os.environ and "S2K_KEY_TABLES_SPLIT" not in os.environ
    yield e
    e.close()


def _both_ladders(eng, oracle, pub, dig, r, s, mode=None, **grouping):
    """the call on comb tables and on window tables: the oracle's verdicts both times; returns them and the comb run's statistics"""
    import secp256k1_voi_amd as S
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    eng.set_key_grouping(S.KEYS_ALWAYS if mode is None else mode, **grouping)
    stats = {}
    try:
        for ladder in (S.LADDER_COMB, S.LADDER_WINDOW):
            eng.set_keyed_ladder(ladder)
            got, st = K._device_run(eng, pub, dig, r, s)
            assert eng.last_keyed_ladder() == ladder, "the call did not build the tables that were asked for"
            assert np.array_equal(got, exp), (ladder, np.nonzero(got != exp)[0][:10])
            assert st["keyed"] + st["general"] == len(pub) and st["keyed"] > 0, (ladder, st)
            stats[ladder] = st
        assert {k: v for k, v in stats[S.LADDER_COMB].items() if k != "complete"} == \
               {k: v for k, v in stats[S.LADDER_WINDOW].items() if k != "complete"}
    finally:
        eng.set_keyed_ladder(S.LADDER_COMB)
        eng.set_key_grouping(S.KEYS_AUTO)
    return exp, stats[S.LADDER_COMB]


MIXED_SIZES = np.array([64] * 40 + [16] * 60 + [5] * 40 + [4] * 50 + [3] * 40 + [1] * 56)


def test_mixed_batch(eng, oracle):
    """keys with 1, 3, 4, 5, 16 and 64 signatures, groups under keys that are no public keys, a seeded tenth damaged"""
    assert MIXED_SIZES.sum() == NSIG
    pub, dig, r, s = K._ragged_batch(eng, 1601, MIXED_SIZES)
    keys, inv, counts = np.unique(pub, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    k16, k5, k64 = (int(np.nonzero(counts == c)[0][0]) for c in (16, 5, 64))
    pub[inv == k16, 63] ^= 1                                                                 # off the curve
    pub[inv == k5, :32] = np.frombuffer((R.P + 5).to_bytes(32, "big"), np.uint8)             # x >= p: not canonical
    pub[inv == k64, 32:] = np.frombuffer(R.P.to_bytes(32, "big"), np.uint8)                  # y = p
    rng = np.random.default_rng(1602)
    hit = rng.permutation(NSIG)[:NSIG // 10]
    for arr, part in zip((r, s, dig), np.array_split(hit, 3)):
        arr[part, rng.integers(0, 32, size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    exp, st = _both_ladders(eng, oracle, pub, dig, r, s)
    assert st["keyed"] == NSIG and st["tables"] == len(MIXED_SIZES)
    assert not exp[(inv == k16) | (inv == k5) | (inv == k64)].any()
    assert NSIG - NSIG // 10 - 85 <= exp.sum() <= NSIG - NSIG // 10          # (16 + 5 + 64 signatures under keys that are none)
    # the default threshold: groups of at least four on the tables, the rest on the general ladder
    import secp256k1_voi_amd as S
    _, st4 = _both_ladders(eng, oracle, pub, dig, r, s, mode=S.KEYS_AUTO)
    assert st4["keyed"] == int(MIXED_SIZES[MIXED_SIZES >= 4].sum()) and st4["general"] == int(MIXED_SIZES[MIXED_SIZES < 4].sum())


def test_random_valid_batch_leaves_the_worklist_empty(eng, oracle):
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = synth_batch(eng, NSIG, 256, seed=1611)
    exp, st = _both_ladders(eng, oracle, pub, dig, r, s)
    assert exp.all() and st["keyed"] == NSIG and st["tables"] == 256
    assert st["complete"] == 0, "a random valid signature reached the complete-formula worklist"


BOUNDARY_HALVES = [1, 3, 2**128 - 1, 2**128 + 1, 2**129 - 1]


def chosen_u2():
    lam = R.LAMBDA
    base = [1, 2, 3, lam, lam + 1, lam - 1, N - 1, (N - 1) // 2, (N + 1) // 2, 2**128 - 1, 2**128 + 1,
            # the comb's own corners: the teeth (bits 19 t of k >> 1), the lead, a full column
            2**19, 2**20, 2**20 + 1, 2**115, 2**116, 2**115 + 1, 2**133 % N, sum(2**(19 * t + 1) for t in range(7)) + 1,
            (1 + lam) * 2**115 % N, (1 + lam) * 2**133 % N]
    # values whose split halves are the boundary halves: u2 = +-b +- c lambda and +-c +- b lambda
    for b in BOUNDARY_HALVES:
        for c in (1, 3, 2**127 - 1):
            for sb in (1, -1):
                for sc in (1, -1):
                    base += [(sb * b + sc * c * lam) % N, (sb * c + sc * b * lam) % N]
    return [v for v in dict.fromkeys(base) if v]


def _rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), np.uint8).reshape(-1, 32).copy()


def test_chosen_scalars(eng, oracle):
    """Signatures of known keys with chosen u2 = r / s: R = (u1 + u2 d) G, r = x(R) mod n, s = r / u2, e = u1 s - random u1
    (valid signatures), u1 = 0 (a zero digest: the generator part is the identity, R = u2 Q) and u1 = -u2 d (R is the identity:
    any r, rejected).  The oracle's verdict in every case, lanes that end on the worklist included."""
    n_keys = 16
    rng = random.Random(1621)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    base = chosen_u2()
    u2 = [base[i % len(base)] for i in range(NSIG)]
    key = [(i // len(base)) % n_keys for i in range(NSIG)]
    kind = [0 if i < NSIG // 2 else 1 + (i & 1) for i in range(NSIG)]                # 0 random u1, 1 u1 = 0, 2 R = identity
    u1 = [rng.randrange(N) if kd == 0 else 0 if kd == 1 else (-b * d[k]) % N for b, k, kd in zip(u2, key, kind)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    Rp = eng.scalar_base_mult_batch(_rows([v or 1 for v in kR]))
    Q = eng.scalar_base_mult_batch(_rows(d))[:, 1:]
    rr = [int.from_bytes(bytes(Rp[i, 1:33]), "big") % N if kR[i] else rng.randrange(1, N) for i in range(NSIG)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    pub = np.ascontiguousarray(Q[key])
    exp, st = _both_ladders(eng, oracle, pub, _rows(ee), _rows(rr), _rows(ss))
    assert st["keyed"] == NSIG and st["tables"] == n_keys
    ok = np.array([kR[i] != 0 and rr[i] != 0 and ss[i] != 0 for i in range(NSIG)])
    assert exp[ok].all() and not exp[~ok].any() and (~ok).sum() >= NSIG // 4
    assert st["complete"] >= int((np.array(kind) == 1).sum()), "the u1 = 0 lanes are the worklist's"


def test_table_cap_sends_groups_to_the_general_ladder(eng, oracle):
    """a cap of 32 tables for 4096 signatures raises the threshold to 128 per key: the sixteen keys that have them get
    tables, the groups of 64 and 16 take the general ladder over the rest list"""
    sizes = np.array([128] * 16 + [64] * 16 + [16] * 64)
    assert sizes.sum() == NSIG
    pub, dig, r, s = K._ragged_batch(eng, 1631, sizes)
    s[::11, 9] ^= 4
    exp, st = _both_ladders(eng, oracle, pub, dig, r, s, max_tables=32)
    assert st["tables"] == 16 and st["keyed"] == 2048 and st["general"] == 2048
    assert 0 < exp.sum() < NSIG


def test_window_path_by_environment_and_split_knob(eng, oracle):
    """S2K_KEYED_LADDER=window at context creation, and S2K_KEY_TABLES_SPLIT at any call, select the window tables"""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = synth_batch(eng, 512, 8, seed=1641)
    r[::5, 3] ^= 2
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    os.environ["S2K_KEYED_LADDER"] = "window"
    try:
        e2 = S.Engine(0)
    finally:
        del os.environ["S2K_KEYED_LADDER"]
    try:
        e2.set_key_grouping(S.KEYS_ALWAYS)
        got, _ = K._device_run(e2, pub, dig, r, s)
        assert np.array_equal(got, exp) and e2.last_keyed_ladder() == S.LADDER_WINDOW
        e2.set_keyed_ladder(S.LADDER_COMB)
        got, _ = K._device_run(e2, pub, dig, r, s)
        assert np.array_equal(got, exp) and e2.last_keyed_ladder() == S.LADDER_COMB
        os.environ["S2K_KEY_TABLES_SPLIT"] = "1"
        try:
            got, _ = K._device_run(e2, pub, dig, r, s)
        finally:
            del os.environ["S2K_KEY_TABLES_SPLIT"]
        assert np.array_equal(got, exp) and e2.last_keyed_ladder() == S.LADDER_WINDOW
        e2.set_key_grouping(S.KEYS_OFF)
        got, _ = K._device_run(e2, pub, dig, r, s)
        assert np.array_equal(got, exp) and e2.last_keyed_ladder() == -1
        with pytest.raises(S.EngineError):
            e2.set_keyed_ladder(7)
    finally:
        e2.close()
