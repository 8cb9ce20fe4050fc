"""Growable key sets, the parts that need no device: the header declares the calls and the binding lists them, the calls
refuse a null set before they touch a device, and the header no longer says that adding keys is not provided."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["s2k_keyset_create_cap", "s2k_keyset_capacity", "s2k_keyset_reserve", "s2k_keyset_append", "s2k_keyset_append_device",
       "s2k_group_keyset_create_cap", "s2k_group_keyset_capacity", "s2k_group_keyset_reserve", "s2k_group_keyset_append"]
S2K_ERR_ARG = -3


def _header():
    with open(os.path.join(ROOT, "include", "secp256k1_voi_amd.h")) as f:
        return f.read()


def test_header_declares_and_binding_lists_the_calls():
    import secp256k1_voi_amd as S
    h = _header()
    for name in NEW:
        assert re.search(r"^(int|size_t)\s+%s\(" % name, h, re.M), name
        assert name in S.EXPORTED_SYMBOLS, name
    assert re.search(r"S2K_ERR_ARG\s*=\s*%d\b" % S2K_ERR_ARG, h)


def test_library_exports_the_calls_and_refuses_a_null_set():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    first = C.c_uint32(7)
    key = (C.c_uint8 * 64)()
    assert lib.s2k_keyset_reserve(None, 100) == S2K_ERR_ARG
    assert lib.s2k_keyset_append(None, 1, key, C.byref(first)) == S2K_ERR_ARG
    assert lib.s2k_keyset_append(None, 0, None, None) == S2K_ERR_ARG
    assert lib.s2k_keyset_append_device(None, 1, None, None) == S2K_ERR_ARG
    assert first.value == 7
    assert lib.s2k_keyset_capacity(None) == 0
    assert lib.s2k_group_keyset_reserve(None, 100) == S2K_ERR_ARG
    assert lib.s2k_group_keyset_append(None, 1, key, None) == S2K_ERR_ARG
    assert lib.s2k_group_keyset_capacity(None) == 0


def test_header_no_longer_says_adding_keys_is_not_provided():
    h = _header()
    assert "adding or removing keys" not in h
    assert not re.search(r"Not (provided|built)[^/]*\badding\b", h)
    assert re.search(r"Not provided[^/]*removing keys", h)
