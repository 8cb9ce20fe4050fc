"""Point sets (s2k_pointset_*) without a device: the table geometry, the big-integer model of the digit recoding, the refusals
that precede every HIP call, and the register budget of the new ladder kernel."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import pointset_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3


def test_geometry():
    import secp256k1_voi_amd as S
    assert S.pointset_geometry(4) == (33, 8, 16896)
    assert S.pointset_geometry(8) == (17, 128, 139264)
    for c in (4, 8):
        pos, ent, nbytes = S.pointset_geometry(c)
        assert pos == M.positions(c) and ent == 1 << (c - 1) and nbytes == pos * ent * 64      # uniform layout, 64-byte entries
    lib = S.load_library()
    out = np.zeros(3, dtype=np.uint64)
    for bad in (0, 5, 16):
        with pytest.raises(ValueError):
            S.pointset_geometry(bad)
        assert lib.s2k_pointset_geometry(bad, out.ctypes.data) == ERR_ARG
    assert lib.s2k_pointset_geometry(4, None) == ERR_ARG


@pytest.mark.parametrize("c", [4, 8])
def test_recoding_model(c):
    rnd = random.Random(900 + c)
    pool = M.boundary_pool()
    half = 1 << (c - 1)
    seen_half = seen_carry = False
    for k in pool + [rnd.getrandbits(128) for _ in range(10000)]:
        ds = M.recode(k, c)
        assert len(ds) == M.positions(c)
        assert sum(d << (c * p) for p, d in enumerate(ds)) == k
        assert all(-half <= d <= half for d in ds) and ds[-1] in (0, 1)
        for d in ds:
            for neg in (False, True):
                w = M.digit_word(d, neg)
                assert w & M.MAG == abs(d) and bool(w & M.NEG) == (d != 0 and (d < 0) != neg) and w < 1 << 16
        if k in pool:
            seen_half = seen_half or any(abs(d) == half for d in ds)
            seen_carry = seen_carry or ds[-1] == 1
    assert seen_half and seen_carry                       # the pool itself holds magnitude 2^(c-1) and the carry digit
    t = (1 << 128) - M.add_constant(c)                     # the threshold is exact
    assert M.recode(t - 1, c)[-1] == 0 and M.recode(t, c)[-1] == 1


def test_split_model_small_scalars_are_their_own_half():
    for k in (int.from_bytes(b"\x80" * 15, "big"), int.from_bytes(b"\x7f" * 16, "big"), 0x80, (1 << 127) - 1):
        assert k < 1 << 127 and M.split(k) == (k, False, 0, False)
    rnd = random.Random(4)
    for _ in range(2000):
        k = rnd.randrange(M.N)
        m1, n1, m2, n2 = M.split(k)
        assert m1 < 1 << 128 and m2 < 1 << 128
        assert ((-m1 if n1 else m1) + (-m2 if n2 else m2) * M.LAM - k) % M.N == 0


def test_refusals_without_a_device():
    import secp256k1_voi_amd as S
    lib = S.load_library()
    pts = np.zeros(65, dtype=np.uint8)
    out = C.c_void_p()
    assert lib.s2k_pointset_create(None, 1, pts.ctypes.data, 4, C.byref(out)) == ERR_ARG and not out.value
    fake = np.zeros(256, dtype=np.uint8)                  # stands for a set: never looked at when the context is null
    k = np.zeros(32, dtype=np.uint8)
    off = np.asarray([0, 1], dtype=np.uint64)
    rec = np.full(65, 0xAB, dtype=np.uint8)
    assert lib.s2k_pointset_multi_scalar_mult_segments(None, fake.ctypes.data, 1, k.ctypes.data, None, 1, off.ctypes.data, rec.ctypes.data) == ERR_ARG
    assert lib.s2k_pointset_multi_scalar_mult_segments_device(None, fake.ctypes.data, 1, k.ctypes.data, None, 1, off.ctypes.data, rec.ctypes.data, None) == ERR_ARG
    assert (rec == 0xAB).all()
    assert lib.s2k_pointset_size(None) == 0 and lib.s2k_pointset_window_bits(None) == 0 and lib.s2k_pointset_device_bytes(None) == 0
    lib.s2k_pointset_destroy(None)
    assert lib.s2k_debug_pointset_entry(None, 0, 0, 1, fake.ctypes.data) == ERR_ARG

    def check(m, n, indexed, offsets):
        o = np.asarray(offsets, dtype=np.uint64)
        return lib.s2k_debug_pointset_check_args(m, n, indexed, len(offsets) - 1, o.ctypes.data)
    assert check(4, 4, 0, [0, 4]) == 0 and check(4, 9, 0, [0, 4, 4, 5, 9]) == 0
    assert check(4, 5, 0, [0, 5]) == ERR_ARG                            # a dense segment longer than the set
    assert b"longer" in lib.s2k_last_error(None)
    assert check(4, 9, 0, [0, 2, 7, 9]) == ERR_ARG
    assert check(4, 5, 1, [0, 5]) == 0                                  # indexed: any length
    for bad in ([1, 5], [0, 3, 2, 5], [0, 4], [0, 6]):                  # the offsets rules of the segmented call
        assert check(8, 5, 0, bad) == ERR_ARG and check(8, 5, 1, bad) == ERR_ARG
    assert lib.s2k_debug_pointset_check_args(8, 0, 0, 0, None) == 0 and lib.s2k_debug_pointset_check_args(8, 5, 0, 1, None) == ERR_ARG


def test_ladder_register_budget():
    """k_ps_ladder has to fit three waves per SIMD, as k_seg_ladder does: at most 168 VGPRs, no spill, no scratch."""
    objdir = os.path.join(ROOT, "secp256k1_voi_amd", "build")
    tool = os.path.join(ROOT, "tools", "kernel_regs.sh")
    if not (os.path.exists(os.path.join(objdir, "pointset.o")) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("objects or llvm tools not available")
    out = subprocess.run(["bash", tool, objdir], capture_output=True, text=True).stdout
    found = {}
    for line in out.splitlines():
        m = re.match(r"\S+\s+(\S+)\s+vgpr=(\d+)\s+sgpr=(\d+)\s+spill=(\d+)\s+scratch=(\d+)", line)
        if m and "k_ps_ladder" in m.group(1):
            found[m.group(1)] = tuple(int(x) for x in m.groups()[1:])
    assert len(found) == 2, sorted(found)                 # both digit widths
    for name, (vgpr, _, spill, scratch) in found.items():
        assert vgpr <= 168 and spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
