"""The index of a key set (s2k_keyset_index_*, s2k_keyset_lookup*, s2k_ecdsa_verify_batch_keyset_bykey*) without a device: the
geometry, the refusals that precede every HIP call, and the binding."""
import ctypes as C

import numpy as np
import pytest

ERR_ARG = -3


def test_geometry():
    import secp256k1_voi_amd as S
    assert S.keyset_index_geometry(1) == (16, 128)
    assert S.keyset_index_geometry(1, 0) == (16, 128)
    assert S.keyset_index_geometry(1000, 0)[0] == 2048
    assert S.keyset_index_geometry(1000, 10) == (1024, 8192)
    assert S.keyset_index_geometry(65536, 0) == (1 << 17, 1 << 20)
    assert S.keyset_index_geometry(1, 1) == (2, 16)
    assert S.keyset_index_geometry(0x0fffffff, 0) == (1 << 29, 1 << 32) and S.keyset_index_geometry(8, 31) == (1 << 31, 1 << 34)
    lib = S.load_library()
    out = np.full(2, 7, dtype=np.uint64)
    for n_keys, log2 in ((1024, 10), (0, 0), (5, 32), (0x10000000, 0), (1 << 31, 31)):
        with pytest.raises(ValueError):
            S.keyset_index_geometry(n_keys, log2)
        assert lib.s2k_keyset_index_geometry(n_keys, log2, out.ctypes.data) == ERR_ARG
    assert (out == 7).all() and b"slots" in lib.s2k_last_error(None)
    assert lib.s2k_keyset_index_geometry(1, 0, None) == ERR_ARG


def test_refusals_without_a_device():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    out = np.full(4, 9, dtype=np.uint64)
    fake = np.zeros(256, dtype=np.uint8)                  # stands for a set: never looked at when the context is null
    buf = np.full(64, 0xAB, dtype=np.uint8)
    assert lib.s2k_keyset_index_info(None, out.ctypes.data) == ERR_ARG and (out == 9).all()
    assert lib.s2k_keyset_index_info(None, None) == ERR_ARG
    assert lib.s2k_keyset_index_create(None, 0) == ERR_ARG
    assert lib.s2k_keyset_lookup(None, None, 1, None, 64, 64, None) == ERR_ARG
    assert lib.s2k_keyset_lookup(None, fake.ctypes.data, 1, buf.ctypes.data, 64, 64, buf.ctypes.data) == ERR_ARG
    assert lib.s2k_keyset_lookup_device(None, None, 1, None, 32, 32, None, None) == ERR_ARG
    assert lib.s2k_keyset_lookup_device(None, fake.ctypes.data, 0, None, 64, 64, None, None) == ERR_ARG
    assert lib.s2k_ecdsa_verify_batch_keyset_bykey(None, None, 1, None, None, None, None, 0, None) == ERR_ARG
    assert lib.s2k_ecdsa_verify_batch_keyset_bykey(None, fake.ctypes.data, 1, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data,
                                                   0, buf.ctypes.data) == ERR_ARG
    assert lib.s2k_ecdsa_verify_batch_keyset_bykey_device(None, None, 0, None, None, None, None, 0, None, None) == ERR_ARG
    assert (buf == 0xAB).all()


def test_binding_exposes_every_new_symbol():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    names = ["s2k_keyset_index_geometry", "s2k_keyset_index_create", "s2k_keyset_index_info", "s2k_keyset_lookup",
             "s2k_keyset_lookup_device", "s2k_ecdsa_verify_batch_keyset_bykey", "s2k_ecdsa_verify_batch_keyset_bykey_device"]
    for name in names:
        assert name in S.EXPORTED_SYMBOLS and getattr(lib, name).argtypes, name
    assert lib.s2k_keyset_lookup.argtypes[4:6] == [C.c_size_t, C.c_size_t]
    for method in ("keyset_lookup", "keyset_lookup_device", "ecdsa_verify_batch_bykey", "ecdsa_verify_batch_bykey_device"):
        assert callable(getattr(S.Engine, method)), method
    assert callable(S.KeySet.index_create) and callable(S.KeySet.index_info) and callable(S.keyset_index_geometry)
