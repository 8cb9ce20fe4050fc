"""The comb ladder's static instruction count, from the code object of the BUILT library (tools/isa_count.py), against the
window ladder's count from the same build and the same tool: 38 additions and 18 doublings instead of 64 and 12 are
564 / 758 = 0.74 of the field products; with the digit extraction the kernel must stay at or below 0.80.  The committed
figures (profiles/*_valu_counts.json: static_comb) must describe the kernel that ships.  No GPU needed."""
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
    return isa_count.static_counts(S.LIB_PATH)


def test_comb_ladder_is_at_most_four_fifths_of_the_window_ladder(live):
    c, k = live["k_verify_fast_comb"], live["k_verify_fast_keyed"]
    print("static VALU: comb %d, window %d, ratio %.4f" % (c["valu_instr_static"], k["valu_instr_static"],
                                                           c["valu_instr_static"] / k["valu_instr_static"]))
    assert c["valu_instr_static"] <= 0.80 * k["valu_instr_static"]


def test_comb_ladder_is_18_doublings_and_38_additions(live):
    c = live["k_verify_fast_comb"]
    # (tools/isa_count.py asserts the trip weights 18 / 38 on the control-flow graph before it counts)
    assert 800 < c["valu_per_trip"]["doubling"] < 1100 and 1300 < c["valu_per_trip"]["addition"] < 1700
    body = 18 * c["valu_per_trip"]["doubling"] + 38 * c["valu_per_trip"]["addition"]
    assert body < c["valu_instr_static"] < body + 6000          # prologue, 19 digit extractions, epilogue
    assert 0.6 < c["mad_u64_u32_per_verify"] / c["valu_instr_static"] < 0.8


def test_committed_comb_counts_describe_the_shipped_kernel(live):
    import test_counts_cpu
    counts, name = test_counts_cpu.newest_counts()
    assert "static_comb" in counts, "%s has no static count of the comb ladder" % name
    ref = counts["static_comb"]["valu_instr_static"]
    got = live["k_verify_fast_comb"]["valu_instr_static"]
    assert abs(got - ref) <= 0.005 * ref, "static count %d, %s says %d - refresh the counts" % (got, name, ref)
    assert abs(live["k_verify_fast_comb"]["mad_u64_u32_per_verify"] - counts["static_comb"]["mad_u64_u32_per_verify"]) <= 0.005 * ref
    pmc = counts.get("k_verify_fast_comb", {}).get("valu_instr_per_signature")
    if pmc is not None:                                           # SQ_INSTS_VALU, once it has been read on a device
        assert abs(got - pmc) <= 0.005 * pmc, "static count %d, PMC in %s %.0f - refresh the counts" % (got, name, pmc)
