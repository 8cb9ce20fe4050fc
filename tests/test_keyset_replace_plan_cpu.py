"""The host-side plan of s2k_keyset_replace / s2k_keyset_remove as a pure function (s2k_debug_keyset_replace_plan; no device):
the argument checks the call makes before it touches anything, the order it works in - the slots ascending - and the number of
pieces, which is all the number of launches depends on.  The slot lists are those of tests/test_gpu_keyset_replace.py."""
import ctypes as C
import os

import numpy as np
import pytest

import secp256k1_voi_amd as S

S2K_OK, S2K_ERR_ARG = 0, -3
NKEYS = 200
RUN = [65, 63, 64]                                                      # step 3: across the 64-lane block, out of order
SCATTER = np.random.default_rng(2401).permutation(NKEYS)[:37]           # step 4: 37 scattered slots


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(S.LIB_PATH):
        S.build()
    return S.load_library()


def _plan(lib, n_live, slots, piece, want_order=True):
    slots = np.ascontiguousarray(slots, dtype=np.uint32)
    m = slots.shape[0]
    order = np.full(max(m, 1), 0xFFFFFFFF, dtype=np.uint32)
    pieces = C.c_uint64(77)
    rc = lib.s2k_debug_keyset_replace_plan(n_live, m, slots.ctypes.data if m else None, piece, order.ctypes.data if want_order else None,
                                           C.addressof(pieces))
    return rc, order[:m], int(pieces.value)


@pytest.mark.parametrize("slots", [RUN, SCATTER, [0], [199], list(range(NKEYS))[::-1]])
def test_order_is_the_slots_sorted(lib, slots):
    slots = np.asarray(slots, dtype=np.uint32)
    rc, order, _ = _plan(lib, NKEYS, slots, 16)
    assert rc == S2K_OK
    assert sorted(order.tolist()) == list(range(len(slots)))              # a permutation of the positions
    assert np.array_equal(slots[order], np.sort(slots))
    assert np.array_equal(S.keyset_replace_plan(NKEYS, slots, 16)["order"], order)


def test_order_of_the_run():
    assert S.keyset_replace_plan(NKEYS, RUN)["order"].tolist() == [1, 2, 0]


@pytest.mark.parametrize("piece", [16, 64])
@pytest.mark.parametrize("m", [1, 16, 17, 200])
def test_piece_counts(lib, m, piece):
    slots = np.random.default_rng(m).permutation(NKEYS)[:m]
    rc, _, pieces = _plan(lib, NKEYS, slots, piece)
    assert rc == S2K_OK and pieces == -(-m // piece)
    rc, untouched, again = _plan(lib, NKEYS, slots, piece, want_order=False)                # (the order is optional)
    assert rc == S2K_OK and again == pieces and (untouched == 0xFFFFFFFF).all()


def test_piece_counts_of_the_device_test(lib):
    assert _plan(lib, NKEYS, SCATTER, 16)[2] == 3 and 37 - 2 * 16 == 5    # three pieces, the last of five
    assert _plan(lib, NKEYS, np.arange(NKEYS), 64)[2] == 4 and NKEYS - 3 * 64 == 8
    assert _plan(lib, NKEYS, SCATTER, 0)[2] == 1                          # no piece size: one piece


def test_refusals(lib):
    for bad in ([NKEYS], [0, NKEYS], [5, 0xFFFFFFFF], [NKEYS + 64, 3]):   # a slot >= n, first or last
        rc, _, pieces = _plan(lib, NKEYS, bad, 16)
        assert rc == S2K_ERR_ARG and pieces == 0, bad
        assert b"slot" in lib.s2k_last_error(None)
    assert _plan(lib, NKEYS, [NKEYS - 1], 16)[0] == S2K_OK
    assert _plan(lib, NKEYS, [7, 7], 16)[0] == S2K_ERR_ARG                # twice, side by side
    assert b"twice" in lib.s2k_last_error(None)
    assert _plan(lib, NKEYS, [7, 150, 3, 99, 7, 12], 16)[0] == S2K_ERR_ARG   # twice, apart in the input
    assert _plan(lib, NKEYS, [7, 150, 3, 99, 7, 12], 16, want_order=False)[0] == S2K_ERR_ARG
    assert _plan(lib, 3, [0, 1, 2, 1], 16)[0] == S2K_ERR_ARG              # more slots than keys: one is named twice
    # NULL slots with m > 0
    assert lib.s2k_debug_keyset_replace_plan(NKEYS, 3, None, 16, None, None) == S2K_ERR_ARG
    with pytest.raises(S.EngineError, match="twice"):
        S.keyset_replace_plan(NKEYS, [1, 2, 1])
    with pytest.raises(ValueError):
        S.keyset_replace_plan(NKEYS, [-1])
    with pytest.raises(ValueError):
        S.keyset_replace_plan(NKEYS, [0.5])


def test_nothing_to_do(lib):
    rc, order, pieces = _plan(lib, NKEYS, [], 16)
    assert rc == S2K_OK and order.size == 0 and pieces == 0
    assert lib.s2k_debug_keyset_replace_plan(NKEYS, 0, None, 0, None, None) == S2K_OK
    assert lib.s2k_debug_keyset_replace_plan(0, 0, None, 16, None, None) == S2K_OK
    p = S.keyset_replace_plan(NKEYS, [], 16)
    assert p["order"].size == 0 and p["pieces"] == 0


def test_calls_refuse_null_without_a_device(lib):
    """the checks in front of every HIP call"""
    one = (C.c_uint32 * 1)(0)
    key = (C.c_uint8 * 64)()
    assert lib.s2k_keyset_replace(None, 1, one, key) == S2K_ERR_ARG
    assert lib.s2k_keyset_replace_device(None, 1, one, None) == S2K_ERR_ARG
    assert lib.s2k_keyset_remove(None, 1, one) == S2K_ERR_ARG
    assert lib.s2k_group_keyset_replace(None, 1, one, key) == S2K_ERR_ARG
    assert lib.s2k_group_keyset_remove(None, 1, one) == S2K_ERR_ARG
    assert lib.s2k_debug_keyset_replace_piece(16) == S2K_OK and lib.s2k_debug_keyset_replace_piece(0) == S2K_OK
