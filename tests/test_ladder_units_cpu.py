"""Where the ladder kernel's instantiations live, read from the sources, without a GPU.

k_verify_fast<MODE> is defined in csrc/verify_fast.h and declared in engine_internal.h; the units that include verify_fast.h
instantiate it explicitly (S2K_LADDER_INSTANCE), launch_ladder (lane_kernels.hip) launches through the declaration, and
engine.hip is host code.  A mode the enum has and no unit instantiates is a link error at best; one that launch_ladder does
not name aborts at the first call; one instantiated twice is compiled twice.

  * the modes of the MODE_* enum, the modes of launch_ladder's switch and the modes instantiated over all units are one set;
  * every mode is instantiated exactly once;
  * engine.hip holds no kernel and no launch.
"""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "secp256k1_voi_amd", "csrc")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        s = f.read()
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", "", s)


def enum_modes():
    """{name: value} of the enum in engine_internal.h that starts with MODE_ECDSA = 0"""
    body = re.search(r"enum\s*\{\s*(MODE_ECDSA\s*=\s*0\b.*?)\}", source("engine_internal.h"), flags=re.S).group(1)
    return {name: int(value) for name, value in re.findall(r"\b(MODE_\w+)\s*=\s*(\d+)", body)}


def switch_modes():
    s = source("lane_kernels.hip")
    body = s[s.index("void launch_ladder("):]
    body = body[body.index("switch (mode)"):body.index("#undef S2K_LADDER")]
    return re.findall(r"\bS2K_LADDER\((MODE_\w+)\)", body)


def instantiated():
    """[(unit, mode)] of every explicit instantiation of k_verify_fast in csrc/"""
    out = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".cpp")):
            continue
        s = source(f)
        out += [(f, mode) for mode in re.findall(r"^\s*S2K_LADDER_INSTANCE\((\w+)\)", s, flags=re.M)]
        assert not re.search(r"\btemplate\s+__global__\s+void\s+k_verify_fast\s*<", s), f"{f}: an instantiation written out by hand"
    return out


def test_enum_switch_and_instantiations_name_the_same_modes():
    modes = enum_modes()
    assert len(modes) == 18 and sorted(modes.values()) == list(range(18))
    sw = switch_modes()
    assert len(sw) == len(set(sw)) and set(sw) == set(modes)
    assert {mode for _, mode in instantiated()} == set(modes)


def test_every_mode_is_instantiated_once():
    inst = instantiated()
    for mode in enum_modes():
        units = [u for u, m in inst if m == mode]
        assert len(units) == 1, (mode, units)
    # the macro is the one explicit instantiation of the template, and the units get the template from the header alone
    header = source("verify_fast.h")
    assert header.count("#define S2K_LADDER_INSTANCE(M)") == 1 and "template __global__ void k_verify_fast<M>(" in header
    for unit in {u for u, _ in inst}:
        assert '#include "verify_fast.h"' in source(unit), unit
    for unit in ("ladder_ecdsa.hip", "ladder_schnorr.hip"):          # a ladder unit: the include and its list, nothing else
        rest = re.sub(r"^\s*S2K_LADDER_INSTANCE\(\w+\)\s*$", "", source(unit), flags=re.M).replace('#include "verify_fast.h"', "")
        assert rest.strip() == "", (unit, rest.strip()[:80])


def test_engine_hip_is_host_code():
    s = source("engine.hip")
    assert "__global__" not in s and "<<<" not in s
    # launch_ladder is the one function that names an instantiation in a launch
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".cpp", ".h")) and f != "lane_kernels.hip":
            assert not re.search(r"k_verify_fast\s*<[^>]*>\s*<<<", source(f)), f
    assert re.search(r"k_verify_fast<M><<<", source("lane_kernels.hip"))
