"""k_key_finish_comb_once on the device (keyed.hip): the comb table's finish kernel that forms the cofactors first and writes
every entry once, against k_key_finish_comb, which parks the sums and fetches them back (S2K_KEY_FINISH_COMB=park, read at
every call).

Every case is one forced keyed call on comb tables run twice, knob unset and =park: the verdicts byte for byte the CPU
oracle's both times, the grouping statistics equal between the two.  Shapes: table counts on the edges of a wave (8 keys)
and of a 256-lane block (32 keys), one batch shown on the CPU to reach every entry with both signs in both halves under
every key, chosen u2, groups under keys that are none beside valid ones in one wave, and a table cap inside a wave."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_comb_model as cm
import test_glv_odd_model as glv
import test_gpu_comb as gc
import test_gpu_keyed as K

pytestmark = pytest.mark.gpu
N = R.N
KNOB = "S2K_KEY_FINISH_COMB"
COUNTS = (1, 7, 8, 9, 31, 32, 33, 65)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    assert KNOB not in os.environ and "S2K_KEYED_LADDER" not in os.environ and "S2K_KEY_TABLES_SPLIT" not in os.environ
    e = S.Engine(0)
    e.set_small_batch_max(0)          # every batch here through the lane kernels: this file is about the tables
    e.set_mid_batch_max(0)
    yield e
    e.close()


def _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s, mode=None, **grouping):
    """the call with the knob unset and with =park: the oracle's verdicts both times, equal statistics; returns them"""
    import secp256k1_voi_amd as S
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    eng.set_key_grouping(S.KEYS_ALWAYS if mode is None else mode, **grouping)
    eng.set_keyed_ladder(S.LADDER_COMB)
    stats = []
    try:
        for park in (False, True):
            if park:
                monkeypatch.setenv(KNOB, "park")
            else:
                monkeypatch.delenv(KNOB, raising=False)
            got, st = K._device_run(eng, pub, dig, r, s)
            assert eng.last_keyed_ladder() == S.LADDER_COMB, "the call did not build comb tables"
            assert np.array_equal(got, exp), (park, np.nonzero(got != exp)[0][:10])
            assert st["keyed"] + st["general"] == len(pub) and st["keyed"] > 0, (park, st)
            stats.append(st)
        assert stats[0] == stats[1]
    finally:
        monkeypatch.delenv(KNOB, raising=False)
        eng.set_key_grouping(S.KEYS_AUTO)
    return exp, stats[0]


@pytest.mark.parametrize("tables", COUNTS)
def test_table_counts_on_wave_and_block_edges(eng, oracle, monkeypatch, tables):
    """`tables` keys of 16 signatures each.  A call of fewer than 256 signatures is not grouped at all (KG_MIN_BATCH), whatever
    the mode: 1, 7, 8 and 9 keys of 16 would build no table.  Those cases are filled up to 256 with signatures of keys that
    sign once and run under KEYS_AUTO (groups of at least four get a table), so that the tables are still exactly `tables`
    keys of 16 signatures; from 31 keys on the batch is the keys alone under KEYS_ALWAYS."""
    import secp256k1_voi_amd as S
    fill = max(0, 256 - 16 * tables)
    pub, dig, r, s = K._ragged_batch(eng, 1200 + tables, np.array([16] * tables + [1] * fill))
    r[::5, 7] ^= 0x20
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s, mode=S.KEYS_AUTO if fill else S.KEYS_ALWAYS)
    assert st["tables"] == tables and st["keyed"] == 16 * tables and st["general"] == fill
    assert 0 < exp.sum() < len(pub)


SEED_COVERAGE = 1231


def _lookups(u2):
    """(half, entry, sign) of the 38 table additions of the comb ladder for u2: the model's digits of the two odd GLV halves,
    the sign as the ladder applies it (test_comb_model.test_ladder_over_the_built_table)"""
    out = set()
    for half, k in enumerate(glv.make_odd(*glv.split_reference(u2))):
        for entry, negative in cm.comb_digits(abs(k)):
            out.add((half, entry, negative != (k < 0)))
    return out


def test_every_entry_of_every_table_is_used(eng, oracle, monkeypatch):
    keys, per_key = 33, 128
    n = keys * per_key
    pub, dig, r, s = K._ragged_batch(eng, SEED_COVERAGE, np.array([per_key] * keys))
    _, inv = np.unique(pub, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    # a seeded tenth is damaged in the digest (u2 = r / s stays what it is); every (half, entry, sign) of every key must be
    # reached by the batch, and by the undamaged nine tenths alone - a wrong entry then turns a valid signature invalid
    rng = np.random.default_rng(SEED_COVERAGE + 1)
    hit = rng.permutation(n)[:n // 10]
    keep = np.ones(n, bool)
    keep[hit] = False
    seen = [set() for _ in range(keys)]
    seen_valid = [set() for _ in range(keys)]
    for i in range(n):
        u2 = int.from_bytes(bytes(r[i]), "big") * pow(int.from_bytes(bytes(s[i]), "big"), -1, N) % N
        lk = _lookups(u2)
        seen[inv[i]] |= lk
        if keep[i]:
            seen_valid[inv[i]] |= lk
    assert all(len(sk) == 2 * 64 * 2 for sk in seen), "SEED_COVERAGE leaves a (half, entry, sign) of a key unused: choose another"
    assert all(len(sk) == 2 * 64 * 2 for sk in seen_valid), "the undamaged signatures alone do not reach every (half, entry, sign): choose another seed"
    dig[hit, rng.integers(0, 32, size=hit.size)] ^= (1 << rng.integers(0, 8, size=hit.size)).astype(np.uint8)
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s)
    assert st["tables"] == keys and st["keyed"] == n
    assert exp[keep].all() and not exp[hit].any()


def test_chosen_scalars(eng, oracle, monkeypatch):
    """the chosen u2 of test_gpu_comb over nine keys (a wave of the finish kernel and one key more): valid signatures with a
    random u1, u1 = 0, and R = the identity (rejected), as there"""
    n_keys = 9
    rng = random.Random(1241)
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


def test_groups_under_invalid_keys(eng, oracle, monkeypatch):
    pub, dig, r, s = K._ragged_batch(eng, 1251, np.array([8] * 40))
    _, inv = np.unique(pub, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    pub[inv == 0, 63] ^= 1                                                                  # off the curve
    pub[inv == 1, :32] = np.frombuffer((R.P + 5).to_bytes(32, "big"), np.uint8)             # x >= p
    pub[inv == 2, 32:] = np.frombuffer(R.P.to_bytes(32, "big"), np.uint8)                   # y = p
    pub[inv == 3] = 0
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s)
    assert exp[inv <= 3].sum() == 0 and exp[inv >= 4].all() and st["keyed"] == len(pub) and st["tables"] == 40


def test_table_cap_of_five(eng, oracle, monkeypatch):
    """five tables: t >= hi cuts inside the first wave of the finish kernel (lanes 40 .. 63 leave)"""
    import secp256k1_voi_amd as S
    pub, dig, r, s = K._ragged_batch(eng, 1261, np.array([64] * 5))
    s[::9, 3] ^= 1
    exp, st = _both_kernels(eng, oracle, monkeypatch, pub, dig, r, s, mode=S.KEYS_AUTO, max_tables=5)   # 320 signatures, 5 tables: groups of >= 64
    assert st["tables"] == 5 and st["keyed"] == 320
    assert 0 < exp.sum() < len(pub)
