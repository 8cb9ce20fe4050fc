"""The comb ladder without the lead point (comb_ladder.hip: k_verify_comb) against the ladder with it (verify_fast.h:
k_verify_fast<MODE_ECDSA_COMB>), both in the BUILT library (tools/isa_count.py on the shipped code object).  No GPU needed.

The first round of the new kernel is the pair sum of its column alone: the lead lookup, jpt29_rescale (2 M),
jpt29_add_affine (8 M + 3 S) and acc.z * h (1 M) are not run - 14 of the column's 20 products.

The bound: 14 products at the static cost of the cheapest product.  That cost is not fixed here, it is read from the same
disassembly: the doubling of k_verify_fast<16> is 7 products (3 M + 4 S; the squarings, the cheapest products, are there)
and a few linear instructions, so its VALU count over 7 is an average that no cheapest product exceeds - 14 times it asks
for at least as much as 14 times the cheapest.  The issue's figure for this, 1 350, is asserted as well."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def live():
    import isa_count
    import secp256k1_voi_amd as S
    if not os.path.exists(isa_count.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    S.build()
    return {"old": isa_count.comb(S.LIB_PATH), "old_schnorr": isa_count.comb(S.LIB_PATH, 17, "SCHNORR_COMB"),
            "new": isa_count.comb_nolead(S.LIB_PATH), "new_schnorr": isa_count.comb_nolead(S.LIB_PATH, True)}


def committed():
    with open(os.path.join(ROOT, "profiles", "r06_valu_counts.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("which", ["new", "new_schnorr"])
def test_loop_trip_weights_are_18_and_18(live, which):
    """isa_count.comb_nolead asserts them on the control-flow graph (every block of the round loop weighs 18: the doubling and
    the column both run 18 times, the peeled round stands in front of the loop); here what it reports"""
    assert live[which]["loop_trips"] == {"column": 18, "doubling": 18}
    t = live[which]["valu_per_trip"]
    assert t["round"] == t["column"] + t["doubling"] and t["addition"] == t["column"] // 2
    # the column is the old kernel's, to a few instructions of scheduling
    old = live["old" if which == "new" else "old_schnorr"]["valu_per_trip"]
    assert abs(t["column"] - old["column"]) <= 0.02 * old["column"], (t, old)
    body = 18 * t["round"]
    assert body < live[which]["valu_instr_static"] < body + 6000


@pytest.mark.parametrize("new,old", [("new", "old"), ("new_schnorr", "old_schnorr")])
def test_the_built_kernel_lost_14_products(live, new, old):
    per_product = live[old]["valu_per_trip"]["doubling"] / 7.0
    diff = live[old]["valu_instr_static"] - live[new]["valu_instr_static"]
    print("%s: static VALU %d, with the lead %d, difference %d; 14 x %.1f = %.0f" %
          (new, live[new]["valu_instr_static"], live[old]["valu_instr_static"], diff, per_product, 14 * per_product))
    assert diff >= 1350
    assert diff >= 14 * per_product
    assert diff <= live[old]["valu_per_trip"]["column"] + 200      # ... and no more than a column and the lead's lookup


@pytest.mark.parametrize("which,key", [("new", "static_comb_nolead"), ("new_schnorr", "static_comb_nolead_schnorr")])
def test_committed_counts_describe_the_shipped_kernel(live, which, key):
    ref = committed()[key]
    got = live[which]
    assert abs(got["valu_instr_static"] - ref["valu_instr_static"]) <= 0.005 * ref["valu_instr_static"], \
        "%s: static count %d, profiles/r06_valu_counts.json says %d - refresh the counts" % (key, got["valu_instr_static"], ref["valu_instr_static"])
    assert abs(got["mad_u64_u32_per_verify"] - ref["mad_u64_u32_per_verify"]) <= 0.005 * got["mad_u64_u32_per_verify"]


def test_register_budget_of_both_instantiations():
    """three waves per SIMD: at most 168 VGPRs, no spill, no scratch, and the 19 KiB of digit columns in LDS"""
    import re
    import subprocess
    objdir = os.path.join(ROOT, "secp256k1_voi_amd", "build")
    if not (os.path.exists(os.path.join(objdir, "comb_ladder.o")) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("objects or llvm tools not available")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), objdir], capture_output=True, text=True).stdout
    found = {}
    for line in out.splitlines():
        mt = re.match(r"\S+\s+(\S+)\s+vgpr=(\d+)\s+sgpr=(\d+)\s+spill=(\d+)\s+scratch=(\d+)\s+lds=(\d+)", line)
        if mt and mt.group(1).startswith("_Z13k_verify_combILb"):
            found[mt.group(1)] = tuple(int(x) for x in mt.groups()[1:])
    assert len(found) == 2, sorted(found)
    for name, (vgpr, _, spill, scratch, lds) in found.items():
        assert vgpr <= 168 and spill == 0 and scratch == 0 and lds == 19 * 256 * 4, (name, vgpr, spill, scratch, lds)


def test_the_counter_pass_agrees_with_the_static_count():
    """k_verify_comb: SQ_INSTS_VALU x 64 / 2^20 of the headline step (profiles/r20_comb_nolead_ab.txt) within 0.5 % of the
    static count, as tests/test_counts_cpu.py asks of the other ladders"""
    c = committed()
    pmc, ref = c["k_verify_comb"]["valu_instr_per_signature"], c["static_comb_nolead"]["valu_instr_static"]
    assert abs(pmc - ref) <= 0.005 * pmc, (pmc, ref)
