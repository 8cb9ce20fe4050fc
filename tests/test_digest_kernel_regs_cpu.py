"""What the built k_digest_messages owns, read from the code object of csrc/digest.hip: no private segment (the word arrays
of the hash cores stay in registers: no spill, no scratch), at most 128 VGPRs, which is four waves per SIMD, and an LDS
block small enough for four workgroups of 256 per CU (160 KiB).  A property of the compiled code: no device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_digest_kernel_register_budget():
    import secp256k1_voi_amd as S
    objdir = os.path.join(ROOT, "secp256k1_voi_amd", "build")
    if not (os.path.exists(os.path.join(objdir, "digest.o")) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("objects or llvm tools not available")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), objdir], capture_output=True, text=True).stdout
    rows = [re.match(r"\S+\s+(\S+)\s+vgpr=(\d+)\s+sgpr=(\d+)\s+spill=(\d+)\s+scratch=(\d+)\s+lds=(\d+)", line) for line in out.splitlines()]
    found = [tuple(int(x) for x in m.groups()[1:]) for m in rows if m and "k_digest_messages" in m.group(1)]
    assert len(found) == 1, out[-2000:]
    vgpr, _, spill, scratch, lds = found[0]
    assert spill == 0 and scratch == 0, found[0]
    assert vgpr <= 128, found[0]
    assert lds == S.digest_caps() and 4 * lds <= 160 * 1024, found[0]
