"""tests/keyset_table_model.py against the oracle: every section's entry is the scalar multiple the model says it is
(oracle.scalar_mult_vartime(m, Q), the oracle's scalar multiplication), the points the model computes with shared inversions
are those multiples, and its geometry is s2k_keyset_geometry's.  No device."""
import random

import numpy as np
import pytest

import keyset_table_model as M
import pyref as R

KEYS = [0xC0FFEE1234567890ABCDEF, R.LAMBDA]        # private scalars: an ordinary one, and the one whose key meets phi
SAMPLE = 300


def _pt65(pt):
    return b"\x04" + pt[0].to_bytes(32, "big") + pt[1].to_bytes(32, "big")


def _multiple(oracle, m, Q):
    out = oracle.scalar_mult_vartime((m % M.N).to_bytes(32, "big"), _pt65(Q))
    assert out[0] == 4
    return (int.from_bytes(out[1:33], "big"), int.from_bytes(out[33:], "big"))


@pytest.fixture(scope="module", params=KEYS, ids=["ordinary", "lambda"])
def tables(request, oracle):
    Q = _multiple(oracle, request.param, R.G)
    return M.KeyTables(Q)


def test_phi_is_lambda(oracle):
    Q = _multiple(oracle, KEYS[0], R.G)
    assert M.phi(Q) == _multiple(oracle, R.LAMBDA, Q)
    assert M.BETA == R.BETA and pow(R.BETA, 3, R.P) == 1 and pow(R.LAMBDA, 3, R.N) == 1


def test_geometry_is_the_library_s():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    assert (M.CHUNKS, M.JOINT, M.JOINT5, M.JOINT6, M.COMB) == (S.KEYSET_CHUNKS, S.KEYSET_JOINT, S.KEYSET_JOINT5, S.KEYSET_JOINT6, S.KEYSET_COMB)
    for layout in M.LAYOUTS:
        out = np.zeros(3, np.uint64)
        assert lib.s2k_keyset_geometry(layout, out.ctypes.data) == 0
        assert int(out[0]) == M.additions_per_signature(layout), layout
        assert int(out[1]) == (M.COMB_SPACING - 1 if layout == M.COMB else 0), layout
        assert int(out[2]) == M.table_bytes_per_key(layout), layout
    g5, g6, g4 = M.joint_geom(M.JOINT5), M.joint_geom(M.JOINT6), M.joint_geom(M.JOINT)
    assert (g5.NE, g5.POS, g5.PER_POS, g5.ENTRIES) == (16, 26, 512, 13314)
    assert (g6.NE, g6.POS, g6.PER_POS, g6.ENTRIES) == (32, 22, 2048, 45058)
    assert (g4.NE, g4.POS, g4.PER_POS, g4.ENTRIES) == (8, 32, 128, 4096)
    assert [M.base_entries(l) for l in M.LAYOUTS] == [258, 258, 258, 258, 66] and [M.joint_entries(l) for l in M.LAYOUTS] == [0, 4096, 13314, 45058, 0]
    # the lead points are where the recodings put them: 2^(W POS) past the last digit, 2^128 for the 32 chunks of 4 bits
    assert g5.W * g5.POS == 130 and g6.W * g6.POS == 132 and 4 * 32 == M.WINDOW_LEAD_LOG2


def _chosen(total, corners, seed):
    idx = set(corners)
    rng = random.Random(seed)
    while len(idx) < min(total, len(corners) + SAMPLE):
        idx.add(rng.randrange(total))
    return sorted(idx)


@pytest.mark.parametrize("layout", [M.CHUNKS, M.COMB], ids=["window", "comb"])
def test_base_entries_are_their_multiples(oracle, tables, layout):
    """every entry of the base tables (258 and 66: all of them)"""
    pts = tables.base(layout)
    assert len(pts) == M.base_entries(layout)
    for idx, pt in enumerate(pts):
        assert pt == _multiple(oracle, M.base_scalar(layout, idx), tables.Q), (layout, idx)


def test_base_scalars_spelled_out():
    assert M.base_scalar(M.CHUNKS, 0) == 1 and M.base_scalar(M.CHUNKS, 7) == 15 and M.base_scalar(M.CHUNKS, 8 * 31 + 7) == 15 << 124
    assert M.base_scalar(M.JOINT6, 9) == 3 << 4
    assert M.base_scalar(M.CHUNKS, 256) == (1 << 128) * (1 + R.LAMBDA) % R.N and M.base_scalar(M.CHUNKS, 257) == (1 << 128) * (1 - R.LAMBDA) % R.N
    assert M.base_scalar(M.COMB, 63) == sum(1 << (19 * t) for t in range(7)) and M.base_scalar(M.COMB, 0) == (1 << 114) - sum(1 << (19 * t) for t in range(6))
    assert M.base_scalar(M.COMB, 64) == (1 << 115) * (1 + R.LAMBDA) % R.N
    g = M.joint_geom(M.JOINT5)
    assert M.joint_scalar(M.JOINT5, 3 * g.PER_POS + 2 * (5 * g.NE + 2) + 1) == ((11 - 5 * R.LAMBDA) << 15) % R.N
    assert M.joint_scalar(M.JOINT, 128 * 31 + 2 * (8 * 7 + 0)) == ((15 + R.LAMBDA) << 124) % R.N
    assert M.joint_geom(M.JOINT6).LEAD == 45056 and M.joint_scalar(M.JOINT6, 45056) == (1 << 132) * (1 + R.LAMBDA) % R.N
    assert M.joint_scalar(M.JOINT6, 45057) == (1 << 132) * (1 - R.LAMBDA) % R.N


@pytest.mark.parametrize("layout", [M.JOINT, M.JOINT5, M.JOINT6], ids=["joint4", "joint5", "joint6"])
def test_joint_entries_are_their_multiples(oracle, tables, layout):
    """all positions for a, b in {0, NE - 1} and both signs, the lead pair, and a seeded sample of the other indices"""
    g = M.joint_geom(layout)
    pts = tables.joint(layout)
    assert len(pts) == g.ENTRIES == M.joint_entries(layout)
    corners = [i * g.PER_POS + 2 * (a * g.NE + b) + s for i in range(g.POS) for a in (0, g.NE - 1) for b in (0, g.NE - 1) for s in (0, 1)]
    corners += list(range(g.LEAD, g.ENTRIES))
    for idx in _chosen(g.ENTRIES, corners, 7000 + layout):
        assert pts[idx] == _multiple(oracle, M.joint_scalar(layout, idx), tables.Q), (layout, idx)
    # a position asked for alone is the same position of the whole table
    some = tables.joint_positions(layout, [0, g.POS - 1])
    assert some[0] == pts[:g.PER_POS] and some[g.POS - 1] == pts[g.LEAD - g.PER_POS:g.LEAD]
    if g.W > 4:
        assert tables.joint_lead(layout) == pts[g.LEAD:]


def test_stored_bytes():
    rng = random.Random(77)
    pts = [(rng.randrange(R.P), rng.randrange(R.P)) for _ in range(5)]
    w = rng.randrange(1, R.P)
    got = M.stored_base(pts, w)
    assert got.shape == (5, 96) and got.dtype == np.uint8
    for k, (x, y) in enumerate(pts):
        sx, sy = x * w * w % R.P, y * pow(w, 3, R.P) % R.P
        assert bytes(got[k, :32]) == R.b32(sx) and bytes(got[k, 32:64]) == R.b32(sy)
        assert bytes(got[k, 64:]) == (R.b32(sx * R.BETA % R.P) if k < 3 else bytes(32))
    assert np.array_equal(M.stored(pts, w), got[:, :64])
    with pytest.raises(AssertionError):
        M.stored(pts, 0)
