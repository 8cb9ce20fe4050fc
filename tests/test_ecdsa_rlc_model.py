"""Whole-batch verification of recoverable ECDSA signatures: the combination in big integers (ecdsa_rlc_model.py), and what
of the feature can be checked without a device - the four entry points in the header, the library and the binding, their
refusal of a null context, and the Python wrappers' argument checks."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import ecdsa_rlc_model as M
import pyref
from pyref import G, N, add, b32, mul, neg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["s2k_ecdsa_batch_verify_rlc", "s2k_ecdsa_batch_verify_rlc_device",
           "s2k_ecdsa_verify_recoverable_batch_bisect", "s2k_ecdsa_verify_recoverable_batch_bisect_device"]


@pytest.fixture(scope="module")
def items():
    return M.make_recoverable_items(6, 2, seed=0xEC0, high_s_every=3)


def coefficients(rng, n):
    return [1] + [rng.randrange(1, 1 << 128) for _ in range(n - 1)]


def test_recoverable_batch_is_good(items, oracle):
    """the helper's v is the one RecoverPublicKey wants: the model and the oracle both return the signing key"""
    assert any(s > N // 2 for _, _, _, s, _ in items) and any(s <= N // 2 for _, _, _, s, _ in items)
    for Q, dg, r, s, v in items:
        assert M.is_good(Q, dg, r, s, v) and M.recover_key(dg, r, s, v) == Q
        assert oracle.ecdsa_recover(dg, b32(r), b32(s), v) == pyref.enc65(Q)
        assert not M.is_good(Q, dg, r, s, v ^ 1)                         # a wrong v: plain-valid, not good
        assert pyref.ecdsa_verify(Q, dg, r, s)
        assert M.is_good(Q, dg, r, s, v, reject_malleable=True) == (s <= N // 2)


def test_good_batch_sums_to_identity(items):
    assert M.combination(items, coefficients(random.Random(1), len(items))) is None


def test_damaged_batch_sums_to_the_weighted_errors(items):
    rng = random.Random(2)
    bad = list(items)
    Q, dg, r, s, v = bad[1]
    bad[1] = (Q, bytes([dg[0] ^ 1]) + dg[1:], r, s, v)                   # a digest bit
    Q, dg, r, s, v = bad[4]
    bad[4] = (bad[3][0], dg, r, s, v)                                    # another valid key
    a = coefficients(rng, len(bad))
    want = None
    for it, c in zip(bad, a):
        want = add(want, mul(c, M.item_error(*it)))
    got = M.combination(bad, a)
    assert got is not None and got == want
    assert [M.item_error(*it) is None for it in bad] == [True, False, True, True, False, True]


def test_cancelling_pair():
    p1, p2 = M.cancelling_pair(0xCA)
    assert not M.is_good(*p1) and not M.is_good(*p2)
    assert M.item_error(*p1) == neg(M.item_error(*p2)) and M.item_error(*p1) is not None
    assert M.combination([p1, p2], [7, 7]) is None
    rng = random.Random(3)
    a1, a2 = rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 128)
    assert a1 != a2 and M.combination([p1, p2], [a1, a2]) is not None


def test_high_x_family(oracle):
    dg, r, s = M.high_x_tuple(0x41)
    assert 1 <= r < pyref.P - N
    for par in (0, 1):
        rec = oracle.ecdsa_recover(dg, b32(r), b32(s), par | 2)
        assert rec is not None
        Q = pyref.dec65(rec)
        assert Q == M.recover_key(dg, r, s, par | 2)
        assert M.is_good(Q, dg, r, s, par | 2) and M.combination([(Q, dg, r, s, par | 2)], [1]) is None
        assert not M.is_good(Q, dg, r, s, par)                           # the same tuple without bit 1
        other = oracle.ecdsa_recover(dg, b32(r), b32(s), par)
        assert other != rec


# ---- the feature itself, as far as it shows without a device ----
def test_entry_points_in_header_library_and_binding():
    import secp256k1_voi_amd as S
    src = open(os.path.join(ROOT, "include", "secp256k1_voi_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(s2k_[a-z0-9_]+)\s*\(", src))
    lib = S.load_library()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in S.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name


def test_null_context_is_refused_without_a_device():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    buf = (C.c_uint8 * 64)()
    res = C.c_int(7)
    p = C.addressof(buf)
    assert lib.s2k_ecdsa_batch_verify_rlc(None, 1, p, p, p, p, p, 0, p, C.byref(res)) == -3          # S2K_ERR_ARG
    assert res.value == 0
    res.value = 7
    assert lib.s2k_ecdsa_batch_verify_rlc_device(None, 1, p, p, p, p, p, 0, p, C.byref(res), None) == -3
    assert res.value == 0
    valid = (C.c_uint8 * 4)(9, 9, 9, 9)
    stats = (C.c_uint32 * 4)(5, 5, 5, 5)
    assert lib.s2k_ecdsa_verify_recoverable_batch_bisect(None, 1, p, p, p, p, p, 0, p, C.addressof(valid), C.addressof(stats)) == -3
    assert lib.s2k_ecdsa_verify_recoverable_batch_bisect_device(None, 1, p, p, p, p, p, 0, p, C.addressof(valid), C.addressof(stats), None) == -3
    assert list(valid) == [9, 9, 9, 9] and list(stats) == [5, 5, 5, 5]


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrappers_check_arguments_before_the_library():
    import secp256k1_voi_amd as S
    eng = object.__new__(S.Engine)               # no context, no device: any call into the library is an error
    eng._lib, eng._h = _NoLibrary(), None
    b = M.make_recoverable_batch(3, 1, seed=5)
    good = (b["pub"], b["digest"], b["r"], b["s"], b["v"])
    for call in (eng.ecdsa_batch_verify_rlc, eng.ecdsa_verify_recoverable_batch):
        for k in range(5):
            args = list(good)
            args[k] = args[k][:2]                                        # lengths disagree
            with pytest.raises(ValueError):
                call(*args)
        for k, w in ((0, 63), (1, 31), (2, 33), (3, 16)):
            args = list(good)
            args[k] = np.zeros((3, w), np.uint8)                         # a row width other than 64 / 32 / 32 / 32
            with pytest.raises(ValueError):
                call(*args)
        with pytest.raises(ValueError):
            call(*good, seed32=bytes(31))
        with pytest.raises(AssertionError):                              # well-formed arguments do reach the library
            call(*good, seed32=bytes(32))
    for call in (eng.ecdsa_batch_verify_rlc_device, ):
        with pytest.raises(ValueError):
            call(3, 0, 0, 0, 0, 0, seed32=bytes(33))
    with pytest.raises(ValueError):
        eng.ecdsa_verify_recoverable_batch_device(3, 0, 0, 0, 0, 0, 0, seed32=bytes(5))
    eng._lib = None
