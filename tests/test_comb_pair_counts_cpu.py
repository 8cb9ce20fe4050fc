"""The comb ladder's column adds its two table entries to each other first (jacobian29.h: coz29_pair_sum): 20 field
products a column instead of 22.  The model counts them, and the BUILT library's comb kernels (tools/isa_count.py on the
shipped code object) must have lost the instructions that go with them.  No GPU needed.

The bound 0.96: a column loses one fe29_mul and one fe29_sqr with their reduction, at least 105 + 69 multiply-adds; at the
project's 143 / 115 instructions for the two, less up to 60 linear ones the pair sum adds, that is >= 198 a column, 19 x 198
= 3.8 k = 4.9 % of the parent's kernel.  0.96 leaves a fifth of that as margin."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the parent commit's kernels (two mixed additions a column), tools/isa_count.py of that commit on its own build:
PARENT_STATIC_ECDSA_COMB = 76661      # k_verify_fast<16>: the figure committed with it (profiles/r06_valu_counts.json: static_comb)
PARENT_STATIC_SCHNORR_COMB = 76207    # k_verify_fast<17>: isa_count.comb(lib, 17, "SCHNORR_COMB") on the parent's library
                                      # (profiles/r13_schnorr_comb_ab.txt section 1 has the same figure)


@pytest.fixture(scope="module")
def live():
    import isa_count
    import secp256k1_voi_amd as S
    if not os.path.exists(isa_count.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    S.build()
    return {16: isa_count.comb(S.LIB_PATH), 17: isa_count.comb(S.LIB_PATH, 17, "SCHNORR_COMB")}


def test_the_model_counts_20_products_a_column():
    import test_comb_pair_model as pm
    pm.test_the_model_counts_20_products()


@pytest.mark.parametrize("mode,parent", [(16, PARENT_STATIC_ECDSA_COMB), (17, PARENT_STATIC_SCHNORR_COMB)])
def test_the_built_kernel_lost_the_two_products(live, mode, parent):
    got = live[mode]["valu_instr_static"]
    print("k_verify_fast<%d>: static VALU %d, parent %d, ratio %.4f" % (mode, got, parent, got / parent))
    assert got <= 0.96 * parent


@pytest.mark.parametrize("mode", [16, 17])
def test_a_column_is_two_additions(live, mode):
    """tools/isa_count.py reports the cost per point addition as half a column; 19 columns and 18 doublings are the body"""
    t = live[mode]["valu_per_trip"]
    assert t["addition"] == t["column"] // 2
    body = 19 * t["column"] + 18 * t["doubling"]
    assert body < live[mode]["valu_instr_static"] < body + 6000
