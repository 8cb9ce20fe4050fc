"""What the built Keccak kernels own, read from the code objects (tools/kernel_regs.sh): k_digest_keccak (csrc/digest.hip)
and k_keccak_address (csrc/address.hip) hold the sponge's 25-lane state in registers - no spill, no scratch - within the 128
VGPRs that __launch_bounds__(256, 4) grants; a state that spilled would still pass every functional test.  And
k_digest_messages, which shares its staging and addressing with the new kernel, is compiled to the figures it had before
that kernel existed.  A property of the compiled code: no device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# k_digest_messages as tools/kernel_regs.sh printed it for the build of commit a080148 (the parent of the Keccak kernels):
# vgpr, spill, scratch
DIGEST_MESSAGES_PARENT = (127, 0, 0)


@pytest.fixture(scope="module")
def kernels():
    objdir = os.path.join(ROOT, "secp256k1_voi_amd", "build")
    if not (os.path.exists(os.path.join(objdir, "digest.o")) and os.path.exists(os.path.join(objdir, "address.o"))
            and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("objects or llvm tools not available")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), objdir], capture_output=True, text=True).stdout
    info = {}
    for line in out.splitlines():
        m = re.match(r"\S+\s+(\S+)\s+vgpr=(\d+)\s+sgpr=(\d+)\s+spill=(\d+)\s+scratch=(\d+)\s+lds=(\d+)", line)
        if m:
            info[m.group(1)] = dict(zip(("vgpr", "sgpr", "spill", "scratch", "lds"), (int(x) for x in m.groups()[1:])))
    return info


def one(kernels, name):
    found = [v for k, v in kernels.items() if name in k]
    assert len(found) == 1, (name, sorted(kernels)[:8])
    return found[0]


@pytest.mark.parametrize("name", ["k_digest_keccak", "k_keccak_address"])
def test_keccak_kernels_keep_the_state_in_registers(kernels, name):
    k = one(kernels, name)
    assert k["spill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)
    assert 4 * k["lds"] <= 160 * 1024, (name, k)          # four workgroups of 256 per CU


def test_digest_messages_is_the_parents_kernel(kernels):
    k = one(kernels, "k_digest_messages")
    assert (k["vgpr"], k["spill"], k["scratch"]) == DIGEST_MESSAGES_PARENT, k
