"""The one-pass build of the per-call key tables (keyed.hip: k_key_finish - co-Z odd multiples, the cofactors from the
eight lanes of a key, the scaling walk) and the affine + affine first addition of k_generator_part.

Every case compares the verdicts with the CPU oracle twice: with k_key_finish, and with the three kernels it replaces
(S2K_KEY_TABLES_SPLIT, read at every call).  Shapes: table counts on the edges of a wave (8 keys) and of a 256-lane
block (32 keys), ragged groups, a table cap, groups under invalid keys, both keyed flows (ECDSA, BIP-340), and one batch
whose digits are shown on the CPU to reach every (chunk, entry, half, sign) of a table.

k_generator_part: the issue asks for u1 whose first two windows select the same or opposite table points.  No such u1
exists (test_coz_model.test_generator_windows_never_meet), so the ZZ = 0 path of xyzz29_add_affine_first is run through
s2k_fp_op_batch_ex (P + P, P - P, operands in their lazy forms), and the kernel with u1 = 0 - every window's digit 0,
the sum ending at infinity - valid and invalid."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import pyref as R
import test_glv_odd_model as glv
import test_gpu_keyed as K
import test_keyed_model as km

pytestmark = pytest.mark.gpu
N = R.N
KNOB = "S2K_KEY_TABLES_SPLIT"
COUNTS = (1, 31, 32, 33, 65)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    e.set_small_batch_max(0)          # every batch here through the lane kernels: this file is about the tables
    e.set_mid_batch_max(0)
    yield e
    e.close()


@contextmanager
def split_kernels(on):
    assert KNOB not in os.environ
    if on:
        os.environ[KNOB] = "1"
    try:
        yield
    finally:
        os.environ.pop(KNOB, None)


def _ecdsa_both(eng, oracle, pub, dig, r, s, tables=None, **grouping):
    """forced grouping, new kernel and old kernels: the oracle's verdicts both times; returns them and the statistics"""
    import secp256k1_voi_amd as S
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    eng.set_key_grouping(S.KEYS_ALWAYS, **grouping)
    try:
        for old in (False, True):
            with split_kernels(old):
                got, st = K._device_run(eng, pub, dig, r, s)
            assert np.array_equal(got, exp), (old, np.nonzero(got != exp)[0][:10])
            assert st["keyed"] + st["general"] == len(pub)
            if tables is not None:
                assert st["tables"] == tables and st["keyed"] > 0, (old, st)
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)
    return exp, st


@pytest.mark.parametrize("tables", COUNTS)
def test_table_counts_on_wave_and_block_edges(eng, oracle, tables):
    sizes = np.array([max(4 + (3 * j) % 5, -(-256 // tables)) for j in range(tables)])      # (batches below 256 are not grouped)
    pub, dig, r, s = K._ragged_batch(eng, 200 + tables, sizes)
    r[::5, 7] ^= 0x20
    exp, _ = _ecdsa_both(eng, oracle, pub, dig, r, s, tables=tables)
    assert 0 < exp.sum() < len(pub)


def test_ragged_groups(eng, oracle):
    sizes = np.array([4, 5, 7, 8, 15, 16, 17, 33, 64, 70] * 3)
    pub, dig, r, s = K._ragged_batch(eng, 301, sizes)
    kind = K._damage(pub, dig, r, s, 302)                       # kinds 0 .. 6 of 24: about a quarter
    assert 0.2 < (kind <= 6).mean() < 0.4
    exp, st = _ecdsa_both(eng, oracle, pub, dig, r, s)
    assert st["keyed"] == len(pub) and 0 < exp.sum() < len(pub)


def test_table_cap_of_five(eng, oracle):
    pub, dig, r, s = K._ragged_batch(eng, 311, np.array([64] * 5))
    s[::9, 3] ^= 1
    import secp256k1_voi_amd as S
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    eng.set_key_grouping(S.KEYS_AUTO, max_tables=5)             # 320 signatures, 5 tables: groups of >= 64
    try:
        for old in (False, True):
            with split_kernels(old):
                got, st = K._device_run(eng, pub, dig, r, s)
            assert np.array_equal(got, exp) and st["tables"] == 5 and st["keyed"] == 320, (old, st)
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)


def test_groups_under_invalid_keys(eng, oracle):
    pub, dig, r, s = K._ragged_batch(eng, 321, np.array([8] * 40))
    _, inv = np.unique(pub, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    pub[inv == 0, 63] ^= 1                                                                  # off the curve
    pub[inv == 1, :32] = np.frombuffer((R.P + 5).to_bytes(32, "big"), np.uint8)             # x >= p
    pub[inv == 2, 32:] = np.frombuffer(R.P.to_bytes(32, "big"), np.uint8)                   # y = p
    pub[inv == 3] = 0
    exp, st = _ecdsa_both(eng, oracle, pub, dig, r, s)
    assert exp[inv <= 3].sum() == 0 and exp[inv >= 4].all() and st["keyed"] == len(pub)


SEED_COVERAGE = 331


def _table_digits(u2):
    """(chunk, entry, half, sign) of the 64 table additions of the keyed ladder for u2 (test_keyed_model's recoding of
    the two odd GLV halves)"""
    out = set()
    for half, k in enumerate(glv.make_odd(*glv.split_reference(u2))):
        for i, w in enumerate(km.nibbles(abs(k))):
            entry = 7 - w if w < 8 else w - 8
            out.add((i >> 2, entry, half, (w < 8) != (k < 0)))
    return out


def test_every_entry_of_a_table_is_used(eng, oracle):
    n = 4096
    pub, dig, r, s = K._ragged_batch(eng, SEED_COVERAGE, np.array([n // 8] * 8))
    seen = set()
    for i in range(n):
        u2 = int.from_bytes(bytes(r[i]), "big") * pow(int.from_bytes(bytes(s[i]), "big"), -1, N) % N
        seen |= _table_digits(u2)
    assert len(seen) == 8 * 8 * 2 * 2, "SEED_COVERAGE leaves a (chunk, entry, half, sign) unused: choose another"
    exp, st = _ecdsa_both(eng, oracle, pub, dig, r, s, tables=8)
    assert exp.all() and st["keyed"] == n


@pytest.mark.parametrize("tables", COUNTS)
def test_bip340_keyed_flow(eng, oracle, tables):
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_schnorr_batch
    n = tables * max(5, -(-256 // tables))
    pk, msgs, sig = synth_schnorr_batch(eng, n, tables, seed=340 + tables)
    sig = sig.copy()
    sig[::4, 40] ^= 1
    exp = np.array([1 if oracle.schnorr_verify(bytes(pk[j]), bytes(msgs[j]), bytes(sig[j])) == 1 else 0 for j in range(n)], dtype=np.uint8)
    assert 0 < exp.sum() < n
    eng.set_key_grouping(S.KEYS_ALWAYS)
    try:
        for old in (False, True):
            with split_kernels(old):
                got = eng.schnorr_verify_batch(pk, msgs, sig)
            st = eng.key_grouping_stats()
            assert np.array_equal(got, exp), (old, np.nonzero(got != exp)[0][:10])
            assert st["tables"] == tables and st["keyed"] == n, (old, st)
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)


# ---- the first addition of k_generator_part -----------------------------------------------------------------------------
def _rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), np.uint8).reshape(-1, 32).copy()


def test_affine_first_addition_formula(eng):
    """xyzz29_add_affine_first through the C-ABI: random pairs, P + P and P - P (flag 0: ZZ3 = ZZZ3 = 0), with the y
    operands in the lazy forms the model allows (+ p limb by limb: [<= 2])"""
    import secp256k1_voi_amd as S
    rng = np.random.default_rng(351)
    pts = [R.mul(int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1, R.G) for _ in range(24)]
    a = pts[:12] * 3
    b = pts[12:] + pts[:12] + [R.neg(p) for p in pts[:12]]
    cols = [_rows([p[0] for p in a]), _rows([p[1] for p in a]), None, _rows([p[0] for p in b]), _rows([p[1] for p in b])]
    for codes in ((0, 0, 0, 0, 0), (0, 1, 0, 0, 1), (0, 1, 0, 0, 0), (0, 0, 0, 0, 1)):
        lazy = sum(c << (4 * j) for j, c in enumerate(codes))
        x, y, flag = eng.fp_op_batch_ex(S.HP_XYZZ_ADD_FIRST, cols, lazy)
        assert list(flag[:12]) == [1] * 12 and not flag[12:].any(), codes
        for i in range(12):
            exp = R.add(a[i], b[i])
            assert (int.from_bytes(bytes(x[i]), "big"), int.from_bytes(bytes(y[i]), "big")) == exp, (codes, i)


def test_generator_part_with_u1_zero(eng, oracle):
    """digest = 0 (and = n): u1 = 0, every window of k_generator_part takes its digit 0 and the sum ends at infinity
    (ZZ = 0 handed to the ladder's last addition).  Valid signatures of this kind (R = u2 Q) and damaged ones."""
    pub, dig, r, s = K._ragged_batch(eng, 361, np.array([64] * 4))
    n, m = len(pub), 48                                           # the first 48 signatures get u1 = 0, the rest stay as they are
    rng = np.random.default_rng(362)
    dig[:m] = 0
    dig[1:m:2] = np.frombuffer(N.to_bytes(32, "big"), np.uint8)
    for i in range(m):
        if i % 4 == 3:
            continue                                              # left as it is: u1 = 0 under a signature that no longer fits
        Q = (int.from_bytes(bytes(pub[i, :32]), "big"), int.from_bytes(bytes(pub[i, 32:]), "big"))
        u2 = int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1
        rr = R.mul(u2, Q)[0] % N
        r[i] = np.frombuffer(rr.to_bytes(32, "big"), np.uint8)
        s[i] = np.frombuffer((rr * pow(u2, -1, N) % N).to_bytes(32, "big"), np.uint8)
    exp, st = _ecdsa_both(eng, oracle, pub, dig, r, s, tables=4)
    assert exp[:m][np.arange(m) % 4 != 3].all() and not exp[3:m:4].any() and exp[m:].all()
    import secp256k1_voi_amd as S
    eng.set_key_grouping(S.KEYS_OFF)
    try:
        got, _ = K._device_run(eng, pub, dig, r, s)
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)
    assert np.array_equal(got, exp)
