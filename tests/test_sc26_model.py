"""CPU model of the 10x26 Montgomery product modulo the group order n (secp256k1_voi_amd/csrc/sc26.h and the generated
sc26_mul_gen.h, tools/gen_sc26_mul.py) that the scalar preparation runs (k_scalar_prep, scalar_prep_one: u1 = e/s,
u2 = r/s).

The committed header is executed as written: its statements are parsed one by one (the v_mad_u64_u32 chains of the
inline asm, the quotient digits m[k], the shifts and the limb stores) and run on Python integers, with every width the
device relies on asserted (32-bit multiplier operands, a 64-bit accumulator that never carries out).  A statement the
interpreter does not know is an error, so an edit of the generator cannot slip past the model.  The results are compared
with a * b * 2^-260 mod n, and the lazy contract is checked on them: output < 2n, limbs 0..8 < 2^26 and limb 9 < 2^23, so
that every output is a legal input again.  The generators of both products must also still reproduce their committed
headers byte for byte.
"""
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "secp256k1_voi_amd", "csrc")
SC26_GEN = os.path.join(CSRC, "sc26_mul_gen.h")

N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
LAMBDA = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
W, L = 26, 10
M26 = (1 << W) - 1
RB = 260
R = 1 << RB
R_INV = pow(R, -1, N)
U32, U64 = 1 << 32, 1 << 64


def limbs(x):
    return [(x >> (W * i)) & M26 for i in range(L - 1)] + [x >> (W * (L - 1))]


def value(v):
    return sum(x << (W * i) for i, x in enumerate(v))


# ---- the interpreter ------------------------------------------------------------------------------------------------
def _read(path=SC26_GEN):
    with open(path) as f:
        return f.read()


def parse_consts(text):
    out = {"SC26_N0INV": int(re.search(r"constexpr uint32_t SC26_N0INV = (0x[0-9a-f]+)u;", text).group(1), 16)}
    for name in ("SC26_N", "SC26_ONE_M", "SC26_R2", "SC26_R3"):
        body = re.search(r"__device__ static const uint32_t %s\[10\] = \{([^}]*)\};" % name, text).group(1)
        out[name] = [int(x.strip().rstrip("u"), 16) for x in body.split(",")]
    return out


def _f26_m():
    with open(os.path.join(CSRC, "fe26.h")) as f:
        return int(re.search(r"constexpr uint32_t F26_M = (0x[0-9A-Fa-f]+)u;", f.read()).group(1), 16)


def _function_body(text, name):
    start = text.index("S2K_DEV sc26 %s(" % name)
    open_ = text.index("{", start)
    depth = 0
    for i in range(open_, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[open_ + 1:i]
    raise AssertionError("unbalanced braces in " + name)


def _statements(body):
    """the body's statements, split at top-level semicolons (a for header keeps its own); preprocessor lines dropped"""
    body = "\n".join(ln for ln in body.splitlines() if not ln.strip().startswith("#"))
    out, depth, cur = [], 0, []
    for ch in body:
        depth += {"(": 1, ")": -1}.get(ch, 0)
        if ch == ";" and depth == 0:
            out.append(" ".join("".join(cur).split()))
            cur = []
        else:
            cur.append(ch)
    assert not "".join(cur).strip(), "trailing text"
    return out


RE_MAD = re.compile(r"v_mad_u64_u32 %0, vcc, %(\d+), %(\d+), %0$")
RE_ASM = re.compile(r'asm\((.*)\s*:\s*"\+&v"\(acc\)\s*:\s*(.*)\s*:\s*"vcc"\)$')
RE_OPND = re.compile(r'"([vs])"\((\w+)(?:\[(\d+)\])?\)')


def compile_fn(text, name, f26_m=None, n0inv=None):
    """the statements of `name` as a list of (operation, argument) steps; raises on a statement it does not know"""
    f26_m = _f26_m() if f26_m is None else f26_m
    n0inv = parse_consts(text)["SC26_N0INV"] if n0inv is None else n0inv
    prog = []
    for st in _statements(_function_body(text, name)):
        m = RE_ASM.match(st)
        if m:
            strings = re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))
            insns = [s.replace("\\n", "").replace("\\t", "").strip() for s in strings]
            opnds = RE_OPND.findall(m.group(2))
            madd = []
            for ins in insns:
                mm = RE_MAD.match(ins)
                assert mm, "unknown instruction: " + ins
                i, j = int(mm.group(1)), int(mm.group(2))
                assert 1 <= i <= len(opnds) and 1 <= j <= len(opnds), ins
                madd.append((opnds[i - 1], opnds[j - 1]))
            prog.append(("mad", madd))
            continue
        if st in ("const uint32_t* a = A.n", "const uint32_t* b = B.n", "uint32_t a2[10]", "uint32_t m[10]", "sc26 r"):
            prog.append(("decl", st))
            continue
        if st == "for (int i = 0; i < 10; ++i) a2[i] = a[i] * 2":
            prog.append(("a2", None))
            continue
        m = re.match(r"const uint32_t (n0 = .*)$", st)
        if m:
            consts = {}
            for part in m.group(1).split(","):
                k, v = part.split("=")
                consts[k.strip()] = int(v.strip().rstrip("u"), 16)
            prog.append(("nconst", consts))
            continue
        if st == "uint64_t acc = 0":
            prog.append(("acc0", None))
            continue
        m = re.match(r"m\[(\d+)\] = \(\(uint32_t\)acc \* SC26_N0INV\) & F26_M$", st)
        if m:
            prog.append(("mdigit", int(m.group(1))))
            continue
        m = re.match(r"acc >>= (\d+)$", st)
        if m:
            prog.append(("shr", int(m.group(1))))
            continue
        m = re.match(r"r\.n\[(\d+)\] = \(uint32_t\)acc & F26_M$", st)
        if m:
            prog.append(("store_masked", int(m.group(1))))
            continue
        m = re.match(r"r\.n\[(\d+)\] = \(uint32_t\)acc$", st)
        if m:
            prog.append(("store", int(m.group(1))))
            continue
        if st == "return r":
            prog.append(("ret", None))
            continue
        raise AssertionError("statement the model does not know: " + st)
    return prog, f26_m, n0inv


class Stats:
    widest = 0


def run(prog, a, b=None, stats=None):
    """execute a compiled body; a, b: 10 limbs each (uint32).  Returns r.n[0..9]."""
    ops, f26_m, n0inv = prog
    assert all(0 <= x < U32 for x in a) and (b is None or all(0 <= x < U32 for x in b))
    env = {"a": list(a), "b": list(b) if b is not None else None, "a2": None, "m": [None] * 10, "r": [None] * 10}
    acc = None

    def get(kind_name_idx):
        kind, nm, idx = kind_name_idx
        if idx == "":
            x = env["nconst"][nm]
            assert kind == "s"
        else:
            x = env[nm][int(idx)]
            assert x is not None, "read before write: %s[%s]" % (nm, idx)
        assert 0 <= x < U32, "32-bit operand"
        return x

    for op, arg in ops:
        if op == "mad":
            assert acc is not None
            for x, y in arg:
                acc = get(x) * get(y) + acc          # v_mad_u64_u32: 32 x 32 + 64 -> 64 (the carry into VCC is never read)
                assert acc < U64, "64-bit accumulator carried out"
                if stats is not None:
                    stats.widest = max(stats.widest, acc.bit_length())
        elif op == "a2":
            env["a2"] = [(x * 2) % U32 for x in env["a"]]
        elif op == "nconst":
            env["nconst"] = arg
        elif op == "acc0":
            acc = 0
        elif op == "mdigit":
            env["m"][arg] = (((acc % U32) * n0inv) % U32) & f26_m
        elif op == "shr":
            acc >>= arg
        elif op == "store_masked":
            env["r"][arg] = (acc % U32) & f26_m
        elif op == "store":
            env["r"][arg] = acc % U32
        elif op == "ret":
            assert all(x is not None for x in env["r"]), "a limb of r is never written"
            return env["r"]
    raise AssertionError("no return")


TEXT = _read()
MONTMUL = compile_fn(TEXT, "sc26_montmul")
MONTSQR = compile_fn(TEXT, "sc26_montsqr")


def check_lazy(r, expect_mod_n):
    v = value(r)
    assert v % N == expect_mod_n % N, "wrong value"
    assert v < 2 * N, "output >= 2n"
    assert all(x < (1 << 26) for x in r[:9]) and r[9] < (1 << 23), "limb out of bounds"


def mm(a, b, stats=None):
    r = run(MONTMUL, limbs(a), limbs(b), stats)
    check_lazy(r, a * b * R_INV)
    return value(r)


def sqr(a, stats=None):
    r = run(MONTSQR, limbs(a), None, stats)
    check_lazy(r, a * a * R_INV)
    return value(r)


# ---- operands --------------------------------------------------------------------------------------------------------
EDGES = [0, 1, 2, N - 1, N, N + 1, 2**256 - 1, 2**256, 2 * N - 1, 2 * N - 2, R % N, R_INV, R_INV + N, (R % N) + N,
         (N - 1) // 2, (N + 1) // 2, 2**128 - 1, 2**128, 2**255, LAMBDA, N - LAMBDA, LAMBDA + N]
# the largest value the limb bounds allow (limbs 0..8 all ones, limb 9 < 2^23): beyond 2n, and still a legal input since
# a * b / R < 2^254 < n keeps the output below 2n
MAX_LIMBS = value([M26] * 9 + [(1 << 23) - 1])


def structured(rng):
    """limb patterns: all ones, single limbs at their bound, n's limbs +- 1, within [0, 2n)"""
    out = []
    nl = limbs(N)
    for fill in (0, 1, M26, 1 << 25, M26 - 1):
        for top in (0, 1, (2 * N >> 234) - 1, (2 * N >> 234) - 2):
            out.append(value([fill] * 9 + [top]))
    for k in range(10):
        for d in (-1, 1):
            v = list(nl)
            v[k] = (v[k] + d) & (M26 if k < 9 else (1 << 23) - 1)
            out.append(value(v))
            out.append(value(v) + N if value(v) < N else value(v))
    for _ in range(40):
        out.append(value([rng.choice((0, 1, M26, M26 - 1, 1 << 25, rng.randrange(1 << 26))) for _ in range(9)] +
                         [rng.randrange(1 << 23)]))
    return [v for v in out if v < 2 * N]


def operands(rng, count):
    pool = EDGES + structured(rng)
    pool += [rng.randrange(2 * N) for _ in range(count)]
    pool += [rng.randrange(N, 2 * N) for _ in range(count // 4)]          # the lazy half, incl. [2^256, 2n)
    pool += [rng.randrange(2**256, 2 * N) for _ in range(count // 8)]
    return pool


# ---- tests -----------------------------------------------------------------------------------------------------------
def test_constants_match_recomputed_values():
    c = parse_consts(TEXT)
    assert c["SC26_N0INV"] == (-pow(N, -1, 1 << 26)) % (1 << 26)
    assert value(c["SC26_N"]) == N and c["SC26_N"] == limbs(N)
    assert value(c["SC26_ONE_M"]) == R % N and c["SC26_ONE_M"] == limbs(R % N)
    assert value(c["SC26_R2"]) == R * R % N and c["SC26_R2"] == limbs(R * R % N)
    assert value(c["SC26_R3"]) == R**3 % N and c["SC26_R3"] == limbs(R**3 % N)
    assert _f26_m() == M26
    for fn in (MONTMUL, MONTSQR):          # the limbs of n each product takes as scalar operands
        (nc,) = [arg for op, arg in fn[0] if op == "nconst"]
        assert [nc["n%d" % j] for j in range(10)] == limbs(N)


def test_interpreter_sees_the_whole_schedule():
    mads = [sum(len(arg) for op, arg in fn[0] if op == "mad") for fn in (MONTMUL, MONTSQR)]
    assert mads[0] == 100 + 100           # a_i b_j and m_i n_j
    assert mads[1] == 55 + 100            # the square's cross terms once, doubled
    for fn in (MONTMUL, MONTSQR):
        kinds = [op for op, _ in fn[0]]
        assert kinds.count("mdigit") == 10 and kinds.count("shr") == 19 and kinds.count("store_masked") == 9
        assert kinds.count("store") == 1 and kinds[-1] == "ret"


def test_montmul_and_montsqr_on_lazy_operands():
    rng = random.Random(260)
    pool = operands(rng, 1200)
    st = Stats()
    for i, a in enumerate(pool):
        b = pool[(i * 7 + 3) % len(pool)]
        assert mm(a, b, st) == mm(b, a, st)                 # both factor orders (the column sums are symmetric)
        sqr(a, st)
        assert run(MONTSQR, limbs(a), None) == run(MONTMUL, limbs(a), limbs(a))      # the same columns, limb for limb
    for a in EDGES:
        for b in EDGES:
            mm(a, b, st)
    # the widest accumulator stays in the budget the generator documents (a column < 20 * 2^52 + 2^38 < 2^57)
    assert st.widest <= 57, st.widest


def test_full_limb_range_stays_below_2n():
    # the limb bounds are the real input contract: any limbs < 2^26 (limb 9 < 2^23), value up to 2^257 - 1
    rng = random.Random(23)
    vals = [MAX_LIMBS, MAX_LIMBS - 1, 2 * N, 2 * N + 1] + [rng.randrange(2 * N, MAX_LIMBS + 1) for _ in range(200)]
    for a in vals:
        for b in (MAX_LIMBS, 2 * N - 1, 1, 0, rng.randrange(MAX_LIMBS + 1)):
            mm(a, b)
            mm(b, a)
        sqr(a)


def test_chain_as_k_scalar_prep_runs_it():
    # acc = 1*R; acc = mm(acc, to_mont(s_i)) for 64 items; the inverse chain then walks back with inv = mm(inv, s_i R)
    rng = random.Random(6)
    for trial in range(6):
        items = [rng.choice((1, N - 1, rng.randrange(1, N), (N + 1) // 2)) for _ in range(64)]
        r2 = value(parse_consts(TEXT)["SC26_R2"])
        acc, prod = R % N, 1
        prefix = []
        for s in items:
            sm = mm(s, r2)                                  # sc26_to_mont: s * R (lazy)
            assert sm % N == s * R % N
            acc = mm(acc, sm)
            prod = prod * s % N
            assert acc % N == prod * R % N
            prefix.append(acc)
        inv = pow(prod, -1, N) * R % N + (N if trial % 2 else 0)   # a lazy inverse (trial odd: in [n, 2n))
        for j in range(63, -1, -1):
            prev = prefix[j - 1] if j else R % N
            s_inv = mm(inv, prev)
            assert s_inv % N == pow(items[j], -1, N) * R % N
            inv = mm(inv, mm(items[j], r2))
    # squarings chained as sc26_sqr_n does
    x = 2 * N - 1
    ref = x
    for _ in range(64):
        x = sqr(x)
        ref = ref * ref * R_INV % N
        assert x % N == ref


def test_model_rejects_a_corrupted_schedule():
    # one operand of one v_mad_u64_u32 changed (b[1] -> b[2] in column 1 of the product)
    bad = TEXT.replace('"v"(a[0]), "v"(b[1]), "v"(a[1]), "v"(b[0]), "v"(m[0]), "s"(n1)',
                       '"v"(a[0]), "v"(b[2]), "v"(a[1]), "v"(b[0]), "v"(m[0]), "s"(n1)', 1)
    assert bad != TEXT
    fn = compile_fn(bad, "sc26_montmul")
    rng = random.Random(1)
    with pytest.raises(AssertionError, match="wrong value"):
        for _ in range(20):
            a, b = rng.randrange(2 * N), rng.randrange(2 * N)
            check_lazy(run(fn, limbs(a), limbs(b)), a * b * R_INV)
    # a shift by one bit too few (after limb 3 of the square)
    cut = TEXT.index("S2K_DEV sc26 sc26_montsqr(")
    store3 = "r.n[3] = (uint32_t)acc & F26_M;\n  acc >>= 26;"
    bad = TEXT[:cut] + TEXT[cut:].replace(store3, store3.replace("26;", "25;"), 1)
    assert bad != TEXT
    fn = compile_fn(bad, "sc26_montsqr")
    with pytest.raises(AssertionError):
        a = rng.randrange(2 * N)
        check_lazy(run(fn, limbs(a)), a * a * R_INV)
    # a statement the model does not know
    with pytest.raises(AssertionError, match="does not know"):
        compile_fn(TEXT.replace("acc >>= 26;", "acc >>= 26; acc += 1;", 1), "sc26_montmul")
    # an instruction the model does not know
    with pytest.raises(AssertionError, match="unknown instruction"):
        compile_fn(TEXT.replace("v_mad_u64_u32 %0, vcc, %1, %2, %0", "v_mad_i64_i32 %0, vcc, %1, %2, %0", 1), "sc26_montmul")


def test_model_rejects_out_of_contract_limbs():
    # limb 9 at 2^27 (an input above the limb bounds): the output leaves [0, 2n)
    big = [M26] * 9 + [1 << 27]
    with pytest.raises(AssertionError, match="output >= 2n|limb out of bounds"):
        r = run(MONTMUL, big, big)
        check_lazy(r, value(big) ** 2 * R_INV)
    # 32-bit limbs overflow the 64-bit accumulator
    with pytest.raises(AssertionError, match="64-bit accumulator"):
        run(MONTMUL, [U32 - 1] * 10, [U32 - 1] * 10)
    # a limb of 2^31 or more wraps in a2 = a * 2 (as in C): the square is then wrong
    a = [M26] * 9 + [1 << 31]
    with pytest.raises(AssertionError):
        check_lazy(run(MONTSQR, a), value(a) ** 2 * R_INV)


@pytest.mark.parametrize("gen,header", [("gen_sc26_mul.py", "sc26_mul_gen.h"), ("gen_fe29_mul.py", "fe29_mul_gen.h")])
def test_generated_header_is_fresh(gen, header):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen)], check=True, capture_output=True,
                         cwd=os.path.join(ROOT, "tools")).stdout
    with open(os.path.join(CSRC, header), "rb") as f:
        committed = f.read()
    assert out == committed, "%s is not what tools/%s emits: regenerate it" % (header, gen)
