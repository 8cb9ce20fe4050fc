"""Where the multiscalar path lives, read from the comment-stripped sources, without a GPU.

msm.hip is the multiscalar core (term arrays in, one point out) with the plain call and the test hook; rlc.hip holds the
whole-batch verifiers, a customer of the core like msm_seg.hip and pointset.hip; msm_terms.h is the term format (device side)
and msm_internal.h the core's host interface.

  * msm.hip names nothing of the whole-batch verifiers, rlc.hip no kernel of the core, and rlc.hip reaches the core only through
    what msm_internal.h declares;
  * the term format has one home: its writers, the curve check and the record classifier are defined in msm_terms.h alone, and
    no unit indexes a record or the zero plane by a literal;
  * msm_core's cut is computed in one function, and the test hook reports what that function returned;
  * engine_internal.h no longer carries the multiscalar declarations.
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "secp256k1_voi_amd", "csrc")
UNITS = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h")))


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        s = f.read()
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", "", s)


def kernels_defined(s):
    """names of the __global__ functions a source defines or declares"""
    return re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(\w+)\s*\(", s)


def kernels_launched(s):
    return re.findall(r"\b(\w+)\s*(?:<[^<>;(){}]*>)?\s*<<<", s)


def function_bodies(s):
    """{name: body} of the functions defined at the top level of a source (or of its namespaces / extern "C" blocks)"""
    out = {}
    for mt in re.finditer(r"\b(\w+)\s*\(", s):
        i, depth = mt.end() - 1, 0
        while i < len(s):
            depth += {"(": 1, ")": -1}.get(s[i], 0)
            i += 1
            if depth == 0:
                break
        rest = s[i:].lstrip()
        if not rest.startswith("{") or mt.group(1) in ("if", "for", "while", "switch", "__launch_bounds__", "__attribute__"):
            continue
        j = s.index("{", i)
        depth, k = 0, j
        while True:
            depth += {"{": 1, "}": -1}.get(s[k], 0)
            k += 1
            if depth == 0:
                break
        out.setdefault(mt.group(1), s[j + 1:k - 1])
    return out


def test_msm_hip_holds_nothing_of_the_verifiers():
    s = source("msm.hip")
    assert not [k for k in kernels_defined(s) + kernels_launched(s) if "rlc" in k]
    assert '"sha256.h"' not in s and "<sys/random.h>" not in s and "<vector>" not in s
    assert "getrandom" not in s
    assert not re.search(r"bip340|BIP-340|schnorr|ecdsa", s, flags=re.I)
    # ... and it has what the issue leaves it: the core's kernels, setup and core, the plain call, the profile calls, the hook
    assert "k_msm_parse" in kernels_defined(s) and "k_msm_debug_fill" in kernels_defined(s)
    bodies = function_bodies(s)
    for f in ("msm_setup", "msm_core", "s2k_internal_msm_enqueue", "s2k_multi_scalar_mult", "s2k_ctx_profile_msm", "s2k_debug_msm_terms"):
        assert f in bodies, f


def test_rlc_hip_is_a_customer_of_the_core():
    s = source("rlc.hip")
    assert not [k for k in kernels_defined(s) + kernels_launched(s) if k.startswith("k_msm_")]
    # the kernels keep their names, in an anonymous namespace with the key type they take by value (their mangled names)
    anon = s[s.index("namespace {"):s.index('extern "C" {')]
    assert anon.count("{") == anon.count("}")          # (the namespace closes before the host code begins)
    for k in ("k_schnorr_rlc_prep", "k_ecdsa_rlc_prep", "k_rlc_key_lift", "k_ecdsa_key_check", "k_rlc_key_terms", "k_schnorr_rlc_sum",
              "k_ecdsa_rlc_leaf", "k_rlc_gather", "k_rlc_save", "k_rlc_mark_valid"):
        assert k in kernels_defined(anon), k
    assert re.search(r"\bstruct\s+rlc_key\b", anon)
    # every msm_* / MSM_* / s2k_internal_msm_* name it uses is declared in msm_internal.h (the core's host interface) or
    # msm_terms.h (the term format); nothing of msm.hip's privates
    declared = set(re.findall(r"\b((?:s2k_internal_)?msm_\w+|MSM_\w+)\b", source("msm_internal.h") + source("msm_terms.h")))
    used = set(re.findall(r"\b((?:s2k_internal_)?msm_\w+|MSM_\w+)\b", s)) - {"msm_internal", "msm_terms"}      # (the include lines)
    assert used <= declared, sorted(used - declared)
    assert '#include "msm_internal.h"' in s and '#include "msm_terms.h"' in s
    assert "ctx->msm_ws" not in s                      # the workspace is the core's: msm_setup carves it, msm_clear zeroes it
    # stage_schnorr is defined before its first use
    first_def = re.search(r"static int stage_schnorr\([^)]*\)\s*\{", s)
    assert first_def and not re.search(r"\bstage_schnorr\(", s[:first_def.start()])
    for unit in ("msm.hip", "rlc.hip", "msm_seg.hip", "pointset.hip"):
        assert '#include "msm_internal.h"' in source(unit), unit


# the record rule written out in a kernel of its own: the test hook's fill kernel, which skips only an all-zero record, and whose
# machine code differed from the parent's with the shared function in front of that test (the head of msm.hip says so)
CLASSIFIER_COPIES = {"msm.hip": "k_msm_debug_fill"}


def test_the_term_format_has_one_home():
    for fn in ("msm_store_term", "msm_store_split", "xy_on_curve_words", "xy_on_curve29", "msm_copy_term", "msm_classify_record",
               "msm_classify_record29"):
        homes = [f for f in UNITS if fn in function_bodies(source(f))]
        assert homes == ["msm_terms.h"], (fn, homes)
    # the flag values have names, and the writers of flags in the multiscalar units use them where they judge a record
    terms = source("msm_terms.h")
    assert re.search(r"TERM_SKIP\s*=\s*0\b", terms) and re.search(r"TERM_FINITE\s*=\s*1\b", terms) and re.search(r"TERM_MALFORMED\s*=\s*2\b", terms)
    for c in ("SCW_WORDS", "TERM_REC_WORDS"):
        assert [f for f in UNITS if re.search(r"constexpr\s+\w+\s+%s\s*=" % c, source(f))] == ["msm_terms.h"], c
    # no unit indexes a record or the zero plane by a literal
    for f in UNITS:
        if not f.endswith(".hip"):
            continue
        for line in source(f).splitlines():
            assert not ("ptw" in line and "* 16)" in line), (f, line.strip())
            assert "(size_t)4 * N" not in line, (f, line.strip())
    # k_rlc_gather and k_rlc_save copy terms through the one function
    bodies = function_bodies(source("rlc.hip"))
    for k in ("k_rlc_gather", "k_rlc_save"):
        assert "msm_copy_term<" in bodies[k] and "uint4" not in bodies[k], k
    # the record rule (0x04, canonical, on the curve; 0x00 the identity): the classifier's two forms, called by k_msm_parse,
    # k_seg_front and k_ps_chain, and the listed copy; the curve equation is written once
    assert "msm_classify_record(" in function_bodies(source("msm.hip"))["k_msm_parse"]
    assert "msm_classify_record29(" in function_bodies(source("msm_seg.hip"))["k_seg_front"]
    assert "msm_classify_record29(" in function_bodies(source("pointset.hip"))["k_ps_chain"]
    assert sum(len(re.findall(r"rhs\.n\[0\]\s*\+=\s*7", source(f))) for f in ("msm_terms.h", "msm.hip", "msm_seg.hip", "pointset.hip")) == 1
    for f in ("msm.hip", "rlc.hip", "msm_seg.hip", "msm_seg_shared.h", "pointset.hip"):
        written_out = [name for name, body in function_bodies(source(f)).items() if re.search(r"rec\[0\]\s*==\s*0x04", body)]
        assert written_out == ([CLASSIFIER_COPIES[f]] if f in CLASSIFIER_COPIES else []), (f, written_out)


def test_one_cut():
    s = source("msm.hip")
    bodies = function_bodies(s)
    # the shortest range: divided by where the workspace is sized (msm_setup), clamped to where the cut is made, nowhere else
    assert [f for f, b in bodies.items() if re.search(r"/\s*MSM_L_MIN\b", b)] == ["msm_setup"]
    assert [f for f, b in bodies.items() if re.search(r"<\s*MSM_L_MIN\b", b)] == ["msm_cut_for"]
    assert sorted(f for f, b in bodies.items() if "MSM_L_MIN" in b) == ["msm_cut_for", "msm_setup"]
    # the ranges and the choice of the reduction are computed in msm_cut_for alone; msm_core runs what it returns
    for pat in (r"\bP\.L_A\s*=", r"\bP\.nlanes\s*=", r"\bfold16\s*=\s*g\.c\s*==\s*16"):
        assert [f for f, b in bodies.items() if re.search(pat, b)] == ["msm_cut_for"], pat
    assert "msm_cut_for(n, m)" in bodies["msm_core"]
    assert sum(src.count('"S2K_MSM_OLD_REDUCE"') for src in map(source, UNITS)) == 1
    # the hook reports the core's values and restates nothing
    hook = bodies["s2k_debug_msm_terms"]
    assert "getenv" not in hook and "msm_lanes_target" not in hook and "FOLD_END" not in hook
    assert re.search(r"geom\[5\]\s*=\s*m\.ran_L_A;", hook) and re.search(r"geom\[6\]\s*=\s*m\.ran_nlanes;", hook)
    assert re.search(r"geom\[7\]\s*=\s*m\.ran_fold16\b", hook)
    core = bodies["msm_core"]
    assert "m.ran_L_A = P.L_A;" in core and "m.ran_nlanes = P.nlanes;" in core and "m.ran_fold16 = fold16;" in core


def test_engine_internal_is_rid_of_the_multiscalar_declarations():
    s = source("engine_internal.h")
    # (the context's own fields msm_ws, msm_prof_ev ... stay: they are its state, freed by engine.hip)
    assert not re.search(r"\b(s2k_internal_msm_\w+|msm_prof_\w+)\s*\(", s)
    assert "MSM_PROF_EV" not in s and "msm_geom" not in s and "struct msm_ws" not in s
    h = source("msm_internal.h")
    for name in ("struct msm_geom", "struct msm_ws", "msm_setup(", "msm_core(", "MSM_DEBUG_TERMS_MAX", "MSM_PROF_EV", "msm_prof_mark(",
                 "s2k_internal_msm_enqueue(", "s2k_internal_msm_reserve("):
        assert name in h, name
    assert "__global__" not in h and "<<<" not in h
    # s2k_internal_point_sub65 is declared in a header, not in the middle of a unit
    assert [f for f in UNITS if re.search(r"s2k_internal_point_sub65\([^)]*\)\s*;", source(f))] == ["engine_internal.h"]
