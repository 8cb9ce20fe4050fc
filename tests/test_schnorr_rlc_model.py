"""The big-integer model of the BIP-340 whole-batch check (schnorr_rlc_model.py) pinned to the oracle's verifier, and what of
the two error-point hooks can be checked without a device: header, library and binding, the refusal of a null context."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import accept_corpus as AC
import ecdsa_rlc_model as EM
import pyref
import schnorr_rlc_model as M
from pyref import G, N, b32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32, 64))
SYMBOLS = ["s2k_debug_schnorr_rlc_point", "s2k_debug_ecdsa_rlc_point"]


@pytest.fixture(scope="module")
def ar(oracle):
    return M.oracle_arith(oracle)


def accepts(oracle, item):
    return oracle.schnorr_verify(bytes(item[0]), bytes(item[1]), bytes(item[2])) == 1       # (-1: the key is no abscissa)


def test_coefficient_against_written_out_digests():
    """SHA-256(KEY || i as 8 bytes, big-endian), computed outside Python: the coefficient is its second half"""
    d1 = "fb76317d6e26241a9626df48efbaa3a628a770304151be369b9fcbc84f40aad1"          # i = 1
    d2 = "47027f9a745eb58e41d5d557182b50af0d04b6da563b9baaecc6555907e57ecd"          # i = 0x123456789
    assert M.coefficient(KEY, 0) == 1
    assert M.coefficient(KEY, 1) == int(d1[32:], 16)
    assert M.coefficient(KEY, 0x123456789) == int(d2[32:], 16)
    assert len({M.coefficient(KEY, i) for i in range(2000)}) == 2000
    assert all(M.coefficient(KEY, i) < 1 << 128 for i in range(2000))


def test_oracle_arithmetic_is_the_group(ar):
    rng = random.Random(1)
    for _ in range(4):
        k, j = rng.randrange(1, N), rng.randrange(1, N)
        A, B = pyref.mul(k, G), pyref.mul(j, G)
        assert ar.base_mult(k) == A and ar.mul(j, A) == pyref.mul(j, A) and ar.add(A, B) == pyref.add(A, B)
    assert ar.add(A, pyref.neg(A)) is None and ar.add(None, A) == A and ar.mul(0, A) is None


def test_item_error_is_the_identity_exactly_where_the_oracle_accepts(oracle, ar):
    """over the accept-rule corpus (valid items, 512 bit flips of r on a fixed R, the two odd-y twins, fillers) ..."""
    c = AC.corpus(oracle)["schnorr"]
    n = len(c["cls"])
    twins = 0
    for i in range(n):
        item = (bytes(c["pk32"][i]), bytes(c["msgs"][i]), bytes(c["sig"][i]))
        E = M.item_error(*item, ar=ar)
        assert (E is None) == bool(c["exp"][i]), (i, c["cls"][i])
        if c["cls"][i] == AC.BIP_ODD:              # s G - e P = -R: the error is -2 R, R the even-y point of r
            R = pyref.lift_x(int.from_bytes(item[2][:32], "big"), 0)
            assert E == pyref.neg(pyref.add(R, R))
            twins += 1
    assert twins == 2


def test_item_error_on_every_damage(oracle, ar):
    """... and over every way to be bad of the device test, on messages of several lengths"""
    items = M.make_items(6, 3, seed=0x340, msg_lens=(32, 1, 65, 200), ar=ar)
    assert all(accepts(oracle, it) and M.item_error(*it, ar=ar) is None and M.in_combination(*it) for it in items)
    for i in (0, 1, 5):
        for name, bad in M.damages(items, i).items():
            E = M.item_error(*bad[i], ar=ar)
            assert not accepts(oracle, bad[i]) and E is not None, (name, i)
            out = name.startswith(("s = ", "r = ", "pk = p", "pk = a non")) or name == "a bit of r that does not lift"
            assert (E is M.OUT) == out == (not M.in_combination(*bad[i])), (name, i)
            assert pyref.schnorr_verify(*bad[i]) is False
    # s = 0 stays in the combination, as in BIP-340 (it is rejected by the equation, not by its range)
    zero = M.with_s(items[2], 0)
    assert M.in_combination(*zero) and M.item_error(*zero, ar=ar) not in (None, M.OUT) and not accepts(oracle, zero)


def test_pure_and_oracle_arithmetic_agree_on_an_error(ar):
    items = M.make_items(2, 2, seed=7, ar=ar)
    bad = M.with_s(items[1], M.parts(items[1])[2] ^ 1)
    want = pyref.neg(G) if M.parts(items[1])[2] & 1 else G                            # s ^ 1 is s - 1 or s + 1
    assert M.item_error(*bad) == want and M.item_error(*bad, ar=ar) == want
    assert M.item_error(*items[0]) is None


def test_error_point_weighs_the_errors(ar):
    items = M.make_items(9, 3, seed=0x99, ar=ar)
    bad = list(items)
    for i in (0, 4, 8):
        bad[i] = M.with_s(items[i], (M.parts(items[i])[2] + i + 1) % N)               # error (i + 1) G
    bad[6] = M.damages(items, 6)["r = a non-abscissa"][6]
    E, status = M.error_point(bad, KEY, ar=ar)
    want = (1 * 1 + M.coefficient(KEY, 4) * 5 + M.coefficient(KEY, 8) * 9) % N
    assert status and E == pyref.mul(want, G)
    assert M.error_point(bad, KEY, 1, 5, ar=ar) == (pyref.mul(M.coefficient(KEY, 4) * 5, G), False)
    assert M.error_point(bad, KEY, 5, 2, ar=ar) == (None, True)
    assert M.error_point(items, KEY, ar=ar) == (None, False)
    assert list(M.in_combination_flags(bad)) == [1, 1, 1, 1, 1, 1, 0, 1, 1]


def test_cancelling_pair(oracle, ar):
    items = M.make_items(2, 1, seed=0xCA, ar=ar)
    delta = random.Random(0xCB).randrange(1, N)
    p1, p2 = M.cancelling_pair(items[0], items[1], delta)
    assert not accepts(oracle, p1) and not accepts(oracle, p2)
    E1, E2 = M.item_error(*p1, ar=ar), M.item_error(*p2, ar=ar)
    assert E1 == ar.base_mult(delta) and E2 == pyref.neg(E1)
    assert ar.add(ar.mul(7, E1), ar.mul(7, E2)) is None                               # equal coefficients: the pair cancels
    for at in ((0, 1), (1, 2), (255, 256)):
        batch = [items[0]] * (at[1] + 1)
        batch[at[0]], batch[at[1]] = p1, p2
        E, status = M.error_point(batch, KEY, ar=ar)
        assert not status and E is not None
        assert E == ar.base_mult((M.coefficient(KEY, at[0]) - M.coefficient(KEY, at[1])) * delta % N)


def test_exceptional_items_are_good(oracle, ar):
    items = M.exceptional_items(6, ar)
    assert all(accepts(oracle, it) for it in items)
    r = lambda i: items[i][2][:32]
    assert r(66) == b32(G[0]) == items[67][0] and r(68) == items[68][0] and r(64) == r(65) and items[64][1] != items[65][1]
    assert len(set(items[:64])) == 1 and r(69) == items[69][0] == b32(G[0])
    assert M.error_point(items, KEY, ar=ar) == (None, False)


def test_ecdsa_error_point(ar):
    items = EM.make_recoverable_items(6, 2, seed=0xEC1, high_s_every=3)
    assert EM.error_point(items, KEY) == (None, False)
    bad = list(items)
    Q, dg, r, s, v = bad[1]
    bad[1] = (Q, bytes([dg[0] ^ 1]) + dg[1:], r, s, v)
    Q, dg, r, s, v = bad[4]
    bad[4] = (Q, dg, r, s, 4)                                                         # v out of range: out of the combination
    assert EM.item_error_with(M.PURE, *bad[1]) == EM.item_error(*bad[1]) == EM.item_error_with(ar, *bad[1])
    coeffs = [M.coefficient(KEY, i) for i in range(6)]
    in_it = [it for i, it in enumerate(bad) if i != 4]
    want = EM.combination(in_it, [c for i, c in enumerate(coeffs) if i != 4])         # the sum as the engine forms it
    assert want is not None
    assert EM.error_point(bad, KEY) == (want, True) == EM.error_point(bad, KEY, ar=ar)
    assert EM.error_point(bad, KEY, 0, 4, ar=ar) == (pyref.mul(coeffs[1], EM.item_error(*bad[1])), False)
    assert EM.error_point(bad, KEY, 2, 4, ar=ar) == (None, True)
    assert EM.from_arrays(EM.to_arrays(items)) == items
    assert [EM.in_combination(*it) for it in bad] == [True, True, True, True, False, True]
    assert not EM.in_combination(*items[2], reject_malleable=True) and EM.in_combination(*items[0], reject_malleable=True)


# ---- the hooks, as far as they show without a device ----
def test_hooks_in_header_library_and_binding():
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


def test_hooks_refuse_a_null_context_without_a_device():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    buf = (C.c_uint8 * 128)()
    p = C.addressof(buf)
    out, status, flags = np.full(65, 9, np.uint8), C.c_uint32(5), np.full(1, 9, np.uint8)
    assert lib.s2k_debug_schnorr_rlc_point(None, 1, p, p, None, 32, p, p, 0, 0, 1, out.ctypes.data, C.byref(status), flags.ctypes.data) == -3
    assert lib.s2k_debug_ecdsa_rlc_point(None, 1, p, p, p, p, p, 0, p, 0, 0, 1, out.ctypes.data, C.byref(status), flags.ctypes.data) == -3
    assert (out == 9).all() and status.value == 5 and flags[0] == 9
    eng = object.__new__(S.Engine)               # no context, no device
    eng._lib, eng._h = None, None
    with pytest.raises(ValueError):
        eng.debug_schnorr_rlc_point(np.zeros((1, 32), np.uint8), [b""], np.zeros((1, 64), np.uint8), bytes(31))
