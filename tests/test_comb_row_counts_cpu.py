"""The wave-per-signature ladder over a COMB key set (small_call.hip: k_verify_row_comb / k_schnorr_row_comb) in the BUILT library,
against its chunk-table siblings from the same disassembly (tools/isa_count.py on the shipped code object): 37 additions of
three layers, 18 doublings of two and 19 conversions - 166 row-product layers on the key part - must come to fewer VALU
instructions per signature wave than k_verify_row_keyset's 64 additions of four layers and the map back (257).  The layer
count says about two thirds; the ratio is printed and the committed one (profiles/r06_valu_counts.json: static_row_comb)
must describe the built kernels.  No GPU needed."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PAIRS = [("k_verify_row_comb", "k_verify_row_keyset"), ("k_schnorr_row_comb", "k_schnorr_row_keyset")]


@pytest.fixture(scope="module")
def live():
    import isa_count
    import secp256k1_voi_amd as S
    if not os.path.exists(isa_count.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    S.build()
    return isa_count.static_counts(S.LIB_PATH)


def committed():
    with open(os.path.join(ROOT, "profiles", "r06_valu_counts.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("new,old", PAIRS)
def test_round_loop_weighs_18(live, new, old):
    """isa_count.row_comb asserts it on the control-flow graph (column 18 stands in front of the loop, no exit in its middle);
    here what it reports, and what the count is made of: 18 rounds and the generator additions, and little else"""
    a = live[new]
    assert a["loop_trips"] == {"round": 18} and (a["key_additions"], a["key_doublings"]) == (37, 18)
    assert a["generator_additions"] == live[old]["generator_additions"] >= 10
    body = 18 * a["valu_per_trip"]["round"] + a["generator_additions"] * a["valu_per_trip"]["generator"]
    assert body < a["valu_instr_static"] < body + 4000
    # the generator part is the sibling's, to a few instructions of scheduling
    assert abs(a["valu_per_trip"]["generator"] - live[old]["valu_per_trip"]["generator"]) <= 8


@pytest.mark.parametrize("new,old", PAIRS)
def test_comb_row_ladder_is_below_the_chunk_row_ladder(live, new, old):
    a, c = live[new], live[old]
    ratio = a["valu_instr_static"] / c["valu_instr_static"]
    print("static VALU per signature wave: %s %d, %s %d, ratio %.4f (row-product layers: 166 / 257 = %.4f on the key part)" %
          (new, a["valu_instr_static"], old, c["valu_instr_static"], ratio, 166 / 257))
    assert a["valu_instr_static"] < c["valu_instr_static"]
    assert a["mad_u64_u32_per_verify"] < c["mad_u64_u32_per_verify"]
    ref = committed()["static_row_comb"][new]
    assert abs(a["valu_instr_static"] - ref["valu_instr_static"]) <= 0.005 * ref["valu_instr_static"], \
        "%s: static count %d, profiles/r06_valu_counts.json says %d - refresh the counts" % (new, a["valu_instr_static"], ref["valu_instr_static"])
    assert abs(ratio - ref["ratio_to_" + old]) <= 0.005, (ratio, ref["ratio_to_" + old])


def _regs(prefixes):
    objdir = os.path.join(ROOT, "secp256k1_voi_amd", "build")
    if not (os.path.exists(os.path.join(objdir, "engine.o")) and os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf")):
        pytest.skip("objects or llvm tools not available")
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_regs.sh"), objdir], capture_output=True, text=True).stdout
    found = {}
    for line in out.splitlines():
        mt = re.match(r"\S+\s+(\S+)\s+vgpr=(\d+)\s+sgpr=(\d+)\s+spill=(\d+)\s+scratch=(\d+)\s+lds=(\d+)", line)
        if mt and mt.group(1).startswith(prefixes):
            found[mt.group(1)] = dict(zip(("vgpr", "sgpr", "spill", "scratch", "lds"), (int(x) for x in mt.groups()[1:])))
    return found


NEW_KERNELS = ("_Z17k_verify_row_comb", "_Z18k_schnorr_row_comb")


def test_no_spill_in_either_new_kernel():
    found = _regs(NEW_KERNELS)
    assert len(found) == 2, sorted(found)
    for name, r in found.items():
        print(name, r)
        assert r["spill"] == 0, (name, r)
    # the block shapes are the siblings': the same registers and the same LDS
    sib = _regs(("_Z19k_verify_row_keyset", "_Z20k_schnorr_row_keyset"))
    for new, old in zip(NEW_KERNELS, ("_Z19k_verify_row_keyset", "_Z20k_schnorr_row_keyset")):
        a = [v for k, v in found.items() if k.startswith(new)][0]
        c = [v for k, v in sib.items() if k.startswith(old)][0]
        assert a["vgpr"] <= c["vgpr"] and a["lds"] == c["lds"], (new, a, c)


def test_no_scratch_in_either_new_kernel():
    """No private segment at all.  The chunk-table siblings own one: the call frames of the __noinline__ scalar helpers
    (sc26.h: sc26_mm, sc26_mont_inv; sha256.h: bip340_challenge) their preparation wave calls.  The new kernels' preparation
    wave takes those helpers expanded in place (scalar_prep_one<true>, schnorr_parse_key<true>) and calls nothing."""
    found = _regs(NEW_KERNELS)
    assert len(found) == 2, sorted(found)
    for name, r in found.items():
        print(name, r)
        assert r["scratch"] == 0, (name, r)


def test_new_kernels_call_nothing_and_touch_no_scratch():
    """the same in the shipped code object: no scratch access and no call anywhere in the new kernels' text"""
    import isa_count
    import secp256k1_voi_amd as S
    if not os.path.exists(isa_count.OBJDUMP):
        pytest.skip("no llvm-objdump in this image")
    S.build()
    for prefix in NEW_KERNELS:
        ins = isa_count.disassemble(S.LIB_PATH, prefix)
        assert len(ins) > 4000, (prefix, len(ins))
        assert not any(i[1].startswith(("scratch_", "s_swappc", "s_call")) for i in ins), prefix


def test_existing_kernels_keep_their_committed_counts(live):
    """k_verify_comb<false> / <true> against profiles/r06_valu_counts.json (as tests/test_comb_nolead_counts_cpu.py asks) and the
    chunk-table row ladders against the figures committed with this ladder (static_row_comb: the parent commit's library
    gives the same), all within 0.5 %"""
    c = committed()
    for kname, key in (("k_verify_comb", "static_comb_nolead"), ("k_verify_comb_schnorr", "static_comb_nolead_schnorr")):
        ref = c[key]["valu_instr_static"]
        assert abs(live[kname]["valu_instr_static"] - ref) <= 0.005 * ref, (kname, live[kname]["valu_instr_static"], ref)
    for kname in ("k_verify_row_keyset", "k_schnorr_row_keyset"):
        ref = c["static_row_comb"][kname]
        for what in ("valu_instr_static", "mad_u64_u32_per_verify", "instructions"):
            assert abs(live[kname][what] - ref[what]) <= 0.005 * ref[what], (kname, what, live[kname][what], ref[what])
