"""Integer model of the generated 9x29 products (secp256k1_voi_amd/csrc/fe29_mul_gen.h) and of their common tail
(fe29.h::fe29_mul_tail), shared by tests/test_fe29_fold32_model.py and tests/test_gpu_fe29_fold32.py.

The model does not restate the schedule: it READS the committed header and executes every statement of a generated
function on Python integers - each v_mad_u64_u32 of each asm chain with the operands the statement names, the masks,
the shifts and the register splits - and refuses any statement it does not know.  The same interpreter runs in two modes:
  * exact: the values are the limbs; the result is compared with arithmetic mod p;
  * bound: the values are upper bounds (every operation is monotone in non-negative operands, a mask is a min).
In both modes every 64-bit accumulator must stay below 2^64 after every multiply-add, every 32-bit value below 2^32,
and the carry of an upper column (high register * 8) below 2^35.  `digits` collects the upper columns' 32-bit digits.
"""
import os
import re

P = 2**256 - 2**32 - 977
L, W = 9, 29
M = (1 << W) - 1
M8 = (1 << 24) - 1
R0, R1 = 0x7A20, 0x100
P_LIMBS = [0x1FFFFC2F, 0x1FFFFFF7] + [M] * 6 + [M8]
U64 = 1 << 64
U32 = 1 << 32
LIMB2_EXCESS = 1 << 12      # "limb 2 may exceed 2^29 by a few thousand" (fe29.h); derivation in test_fe29_fold32_model.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "secp256k1_voi_amd", "csrc", "fe29_mul_gen.h")

# name -> (operand names in call order, value as a function of the operands' integer values)
FORMS = {
    "fe29_mul": ("AB", lambda A, B: A * B),
    "fe29_sqr": ("A", lambda A: A * A),
    "fe29_mul_add_mul": ("ABCD", lambda A, B, C, D: A * B + C * D),
    "fe29_mul_add_sqr": ("ABC", lambda A, B, C: A * B + C * C),
    "fe29_mul_plus": ("ABE", lambda A, B, E: A * B + E),
    "fe29_sqr_plus": ("AE", lambda A, E: A * A + E),
}


def value(n):
    return sum(x << (W * i) for i, x in enumerate(n))


def from_int(v):
    return [(v >> (W * i)) & M for i in range(L - 1)] + [v >> (W * (L - 1))]


def units_bound(w):
    """limb bounds of a value of w units (fe29.h)"""
    return [int(w * (1 << W))] * 8 + [int(w * ((1 << 24) + 16))]


def lazy_form(v, code):
    """ops.hip::fe29_lazy_form on the limbs of a canonical value: bit 2 = borrow-spread, bits 1:0 = multiples of p added"""
    n = from_int(v)
    if code & 4:
        for i in range(8):
            if n[i + 1] > 0:
                n[i + 1] -= 1
                n[i] += 1 << W
    k = code & 3
    return [x + k * p for x, p in zip(n, P_LIMBS)]


def functions(path=HEADER):
    """name -> body text of every generated product"""
    with open(path) as f:
        text = f.read()
    out = {}
    for m in re.finditer(r"^S2K_DEV fe29 (\w+)\(([^)]*)\) \{\n(.*?)^\}\n", text, re.S | re.M):
        if m.group(1) in FORMS:
            out[m.group(1)] = m.group(3)
    assert set(out) == set(FORMS), sorted(out)
    return out


def mul_tail(t, c, h, bound=False):
    """fe29.h::fe29_mul_tail: h is the high register of column 16's sum"""
    def trunc(x):
        return min(x, U32 - 1) if bound else x & (U32 - 1)

    def mask(x, m):
        return min(x, m) if bound else x & m
    assert h < U32 and t[8] < U32
    c += t[8]
    c += h * (R0 << 3)
    assert c < U64, "64-bit accumulator (tail, column 8)"
    r8 = mask(trunc(c), M8)
    c >>= 24
    assert c < U32, "fold count does not fit 32 bits"
    k0, k1 = R0 >> 5, R1 >> 5
    e = t[0] + c * k0
    assert e < U64
    e += h * (k0 << 16)
    assert e < U64, "64-bit accumulator (tail, limb 0)"
    r0 = mask(trunc(e), M)
    e >>= W
    e += t[1]
    e += c * k1
    assert e < U64
    e += h * (k1 << 16)
    assert e < U64, "64-bit accumulator (tail, limb 1)"
    r1 = mask(trunc(e), M)
    e >>= W
    assert e < U32
    r2 = t[2] + e
    assert r2 < U32
    return [r0, r1, r2] + list(t[3:8]) + [r8]


_ASM = re.compile(r'asm\((.*?)\n\s*: ((?:"[=+]&?v"\(\w+\)(?:, )?)+)\n\s*: (.*?)\n\s*: "vcc"\);\n', re.S)
_OUT = re.compile(r'"([=+]&?)v"\((\w+)\)')
_INSN = re.compile(r"v_mad_u64_u32 %(\d+), vcc, %(\d+), (%\d+|8), (0|%\d+)")
_OPERAND = re.compile(r'"[vsn]"\(([^)]*)\)')


def run(body, operands, bound=False, digits=None):
    """Executes one generated function on `operands` (dict A.. -> 9 limbs, or 9 limb bounds with bound=True)."""
    env = {k: list(v) for k, v in operands.items()}
    env.update(F29_R0=R0, F29_R1=R1)
    for v in operands.values():
        assert len(v) == L and all(0 <= x < U32 for x in v), "32-bit limb"
    pending_carry = [None]    # the high register read last: the next upper chain must start from it times 8

    def ev(expr):
        expr = expr.strip()
        if expr.isdigit():
            return int(expr)
        m = re.fullmatch(r"(\w+)(?:\.n)?\[(\d+)\]", expr)
        if m:
            return env[m.group(1)][int(m.group(2))]
        return env[expr]

    def trunc(x):
        return min(x, U32 - 1) if bound else x & (U32 - 1)

    pos = 0
    while pos < len(body):
        if body.startswith("  asm(", pos):
            m = _ASM.match(body, pos + 2)
            assert m, body[pos:pos + 200]
            insns, outs, ops = m.group(1), _OUT.findall(m.group(2)), _OPERAND.findall(m.group(3))
            nout = len(outs)
            vals = [None] * nout + [ev(o) for o in ops]     # the inputs are read before the statement writes anything
            acc = [env.get(var) if mode[0] == "+" else None for mode, var in outs]
            # an output without the early-clobber mark may share registers with inputs that are parts of its own incoming
            # value: such inputs (u, h of d) must be read no later than the instruction that first writes it
            written, shared = set(), {}
            for io, (mode, var) in enumerate(outs):
                if "&" not in mode:
                    assert var == "d" and mode == "+"
                    shared.update({nout + j: io for j, o in enumerate(ops) if o in ("u", "h")})
            lines = _INSN.findall(insns)
            assert len(lines) == insns.count("v_mad_u64_u32"), insns
            for io, ia, ib, add in lines:
                io, ia = int(io), int(ia)
                assert io < nout <= ia
                a = vals[ia]
                for used in (ia,) + ((int(ib[1:]),) if ib != "8" else ()):
                    assert shared.get(used) not in written, "an input that may live in d's registers is read after d is written"
                written.add(io)
                if ib == "8":
                    assert add == "0" and outs[io][1] == "d" and ops[ia - nout] == "h" and pending_carry[0] is not None
                    b = 8
                    assert a * 8 < 1 << 35, "carry of an upper column"
                    pending_carry[0] = None
                else:
                    assert int(ib[1:]) >= nout
                    b = vals[int(ib[1:])]
                assert a < U32 and b < U32, "32-bit operand"
                if add == "0":
                    assert acc[io] is None, "an accumulator is overwritten"
                    acc[io] = a * b
                else:
                    assert int(add[1:]) == io and acc[io] is not None, "accumulator read before it is written"
                    acc[io] += a * b
                assert acc[io] < U64, "64-bit accumulator overflow in " + outs[io][1]
            for (mode, var), x in zip(outs, acc):
                assert x is not None
                env[var] = x
            pos = m.end()
            continue
        end = body.index("\n", pos)
        line = body[pos:end].strip()
        pos = end + 1
        if not line or line == "#pragma unroll" or line in ("uint64_t d, c;", "uint32_t t[9];"):
            if line == "uint32_t t[9];":
                env["t"] = [None] * 9
            continue
        m = re.fullmatch(r"const uint32_t\* (\w+) = (\w)\.n;", line)
        if m:
            env[m.group(1)] = env[m.group(2)]
            continue
        m = re.fullmatch(r"uint32_t (\w+)\[9\];", line)
        if m:
            env[m.group(1)] = [None] * 9
            continue
        m = re.fullmatch(r"for \(int i = 0; i < 9; \+\+i\) (\w+)\[i\] = (\w+)\[i\] \* 2;", line)
        if m:
            env[m.group(1)] = [2 * x for x in env[m.group(2)]]
            assert all(x < U32 for x in env[m.group(1)]), "doubled limb does not fit 32 bits"
            continue
        if line == "const uint32_t R0 = F29_R0, R1 = F29_R1;":
            env["R0"], env["R1"] = R0, R1
            continue
        if line == "uint32_t u, h;":
            continue
        m = re.fullmatch(r"t\[(\d)\] = \(uint32_t\)(\w) & F29_M;", line)
        if m:
            env["t"][int(m.group(1))] = min(env[m.group(2)], M) if bound else env[m.group(2)] & M
            continue
        m = re.fullmatch(r"(\w) >>= 29;", line)
        if m:
            env[m.group(1)] >>= W
            continue
        if line == "u = (uint32_t)d;":
            env["u"] = trunc(env["d"])
            if digits is not None:
                digits.append(env["u"])
            continue
        if line == "h = (uint32_t)(d >> 32);":
            assert pending_carry[0] is None, "a high register was dropped"
            env["h"] = env["d"] >> 32
            pending_carry[0] = env["h"]
            del env["d"]            # the column sum is spent: the next chain must write it anew
            continue
        if line == "return fe29_mul_tail(t, c, h);":
            assert pending_carry[0] == env["h"]
            return mul_tail(env["t"], env["c"], env["h"], bound)
        raise AssertionError("statement the model does not know: " + line)
    raise AssertionError("no return")


def check_result(r, exact):
    """1 unit, limb 2 allowed LIMB2_EXCESS more; congruent to `exact` (None: bounds only)"""
    assert all(r[i] <= M for i in (0, 1, 3, 4, 5, 6, 7)) and r[8] <= M8 and r[2] <= M + LIMB2_EXCESS, r
    if exact is not None:
        assert value(r) % P == exact % P
