"""The wave-per-signature key-set ladder's static instruction count, from the code object of the BUILT library
(tools/isa_count.py): 64 additions on the key's isomorphic curve and the generator part must come to fewer VALU instructions
per signature wave than k_verify_row's table build, 128 doublings and 64 additions from the same build and the same tool.
No GPU needed."""
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


def test_static_counts_list_the_new_kernels(live):
    assert "k_verify_row_keyset" in live and "k_schnorr_row_keyset" in live and "k_verify_row" in live
    for name in ("k_verify_row_keyset", "k_schnorr_row_keyset"):
        assert live[name]["key_additions"] == 64 and live[name]["generator_additions"] >= 10


def test_keyset_row_ladder_is_below_the_general_row_ladder(live):
    a, c = live["k_verify_row_keyset"], live["k_verify_row"]
    print("static VALU per signature wave: key set %d, general %d, ratio %.4f" % (a["valu_instr_static"], c["valu_instr_static"],
                                                                                   a["valu_instr_static"] / c["valu_instr_static"]))
    assert a["valu_instr_static"] < c["valu_instr_static"]
    # what the count is made of: 32 chunk rounds and the generator additions, and little else
    body = 32 * a["valu_per_trip"]["chunk"] + a["generator_additions"] * a["valu_per_trip"]["generator"]
    assert body < a["valu_instr_static"] < body + 4000
