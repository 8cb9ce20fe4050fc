"""The BIP-340 comb ladder's static instruction count, from the code object of the BUILT library (tools/isa_count.py), against
the BIP-340 window ladder's count from the same build and the same tool.  As for the ECDSA pair (test_comb_counts_cpu.py): 38
additions and 18 doublings instead of 64 and 12 are 564 / 758 = 0.74 of the field products; with the digit extraction the kernel
must stay at or below 0.80.  k_verify_fast<MODE_SCHNORR_COMB> serves the calls' tables and comb key sets alike (a test on
kg.key_bytes that is uniform over the launch): there is no second instantiation to compare.  No GPU needed."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def counts():
    import isa_count
    import secp256k1_voi_amd as S
    if not os.path.exists(isa_count.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    S.build()
    # (comb() asserts the trip weights 18 / 38 on the control-flow graph before it counts, keyed() 12 / 64)
    return {"comb": isa_count.comb(S.LIB_PATH, 17, "SCHNORR_COMB"), "window": isa_count.keyed(S.LIB_PATH, 6, "SCHNORR_KEYED"),
            "ecdsa_comb": isa_count.comb(S.LIB_PATH), "all": isa_count.static_counts(S.LIB_PATH)}


def test_schnorr_comb_is_18_doublings_and_38_additions(counts):
    c = counts["comb"]
    assert 800 < c["valu_per_trip"]["doubling"] < 1100 and 1300 < c["valu_per_trip"]["addition"] < 1700
    body = 18 * c["valu_per_trip"]["doubling"] + 38 * c["valu_per_trip"]["addition"]
    assert body < c["valu_instr_static"] < body + 6000          # prologue, 19 digit extractions, epilogue
    assert 0.6 < c["mad_u64_u32_per_verify"] / c["valu_instr_static"] < 0.8


def test_schnorr_comb_is_at_most_four_fifths_of_the_schnorr_window_ladder(counts):
    c, k = counts["comb"]["valu_instr_static"], counts["window"]["valu_instr_static"]
    print("static VALU: BIP-340 comb %d, BIP-340 window %d, ratio %.4f" % (c, k, c / k))
    assert c <= 0.80 * k


def test_static_counts_lists_the_new_kernels_and_keeps_the_old(counts):
    a = counts["all"]
    assert a["k_verify_fast_schnorr_comb"] == counts["comb"] and a["k_verify_fast_schnorr_keyed"] == counts["window"]
    assert a["k_verify_fast_comb"] == counts["ecdsa_comb"]
    for key in ("k_verify_fast", "k_verify_fast_keyed", "k_verify_fast_comb", "k_verify_fast_keyset", "k_verify_fast_keyset_joint",
                "k_verify_fast_keyset_joint5", "k_verify_fast_keyset_joint6"):
        assert key in a
