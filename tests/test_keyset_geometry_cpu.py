"""s2k_keyset_geometry: what a key-set layout costs per signature (table additions, doublings) and per key (table bytes).  A pure
host function - no device, no context - whose values come from the geometries the kernels are built on; the figures here are
the ones the header and DESIGN.md state.  The comb layout is the small one: 10 KiB per key, 3.6 times below the chunk tables."""
import numpy as np
import pytest

ERR_ARG = -3
CHUNK_BYTES = 288 * 128
EXPECTED = {
    "KEYSET_CHUNKS": (64, 0, 36864),
    "KEYSET_JOINT": (32, 0, 36864 + 327680),
    "KEYSET_JOINT5": (26, 0, 36864 + (26 * 512 + 2) * 64),
    "KEYSET_JOINT6": (22, 0, 36864 + (22 * 2048 + 2) * 64),
    "KEYSET_COMB": (38, 18, 10240),
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_geometry_of_every_layout(name):
    import secp256k1_voi_amd as S
    layout = getattr(S, name)
    out = np.zeros(3, dtype=np.uint64)
    assert S.load_library().s2k_keyset_geometry(layout, out.ctypes.data) == 0
    assert tuple(int(x) for x in out) == EXPECTED[name]
    assert S.keyset_geometry(layout) == EXPECTED[name]


def test_layout_numbers_and_the_size_ratio():
    import secp256k1_voi_amd as S
    assert (S.KEYSET_AUTO, S.KEYSET_CHUNKS, S.KEYSET_JOINT, S.KEYSET_JOINT5, S.KEYSET_JOINT6, S.KEYSET_COMB) == (0, 1, 2, 3, 4, 5)
    assert CHUNK_BYTES == EXPECTED["KEYSET_CHUNKS"][2]
    chunks, comb = S.keyset_geometry(S.KEYSET_CHUNKS), S.keyset_geometry(S.KEYSET_COMB)
    assert chunks[2] * 10 == comb[2] * 36                                # 3.6 times smaller
    # field products of a ladder: 11 per Jacobian mixed addition and 7 per doubling against 10 per XYZZ addition
    assert comb[0] * 11 + comb[1] * 7 == 544 < chunks[0] * 10


def test_auto_and_unknown_layouts_are_refused():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    out = np.full(3, 77, dtype=np.uint64)
    for bad in (S.KEYSET_AUTO, 6, -1, 1000):
        assert lib.s2k_keyset_geometry(bad, out.ctypes.data) == ERR_ARG
        assert out.tolist() == [77, 77, 77]
        with pytest.raises(ValueError):
            S.keyset_geometry(bad)
    assert lib.s2k_keyset_geometry(S.KEYSET_COMB, None) == ERR_ARG
