"""The 9x29 products with 32-bit upper digits (tools/gen_fe29_mul.py, fe29.h::fe29_mul_tail), on the CPU.

Upper columns 9..16 of a product are split on the register boundary: the digit is the low 32 bits of the column sum, the
carry into the next column its high 32 bits times 8.  tests/fe29_fold32_model.py executes the statements of the committed
generated header on integers; here that model is run
  (a) on random and extremal lazy operands at the unit budgets of fe29.h, against arithmetic mod p;
  (b) on limb BOUNDS at those budgets: every accumulator < 2^64, every carry hi * 8 < 2^35, result of 1 unit;
  (c) past the budget, where it must report an overflow;
and (d) the committed header is what the generator emits.

Bound of limb 2 (LIMB2_EXCESS = 2^12), from the formats and not from a run: column 16 holds one product per fused term, of
limbs 8 (<= w (2^24 + 16)), so at most 7.8 (2^24 + 16)^2 < 2^51 plus a carry < 2^35; its high register h is below 2^19.
The fold count c_lo is (carry < 2^36, digit < 2^29, u R1 < 2^40, h 8 R0 < 2^37) >> 24 < 2^17.  Limb 0's sum is below
2^29 + 2^17 * 977 + 2^19 * 977 * 2^16 < 2^45, so it carries < 2^16 into limb 1, whose sum is below
2^29 + 2^16 + 2^17 * 8 + 2^19 * 8 * 2^16 < 2^38.1 + 2^29.1: it carries less than 2^9.2 + 2 < 2^12 into limb 2.
"""
import os
import random
import subprocess
import sys

import pytest

import fe29_fold32_model as F
from fe29_fold32_model import FORMS, L, M, M8, P, P_LIMBS, U32, W, units_bound, value

FUNCS = F.functions()

# unit budgets: per form, the units of the operands in call order; the products of the factors' units, summed over the
# fused terms, are <= 7.8 (fe29.h).  An addend E is any value whose limbs fit 32 bits (7.9 units), as the formulas use it.
BUDGETS = {
    "fe29_mul": [(1, 1), (2, 2), (2, 3.9), (3.9, 2), (1, 7.8), (7.8, 1), (2.79, 2.79)],
    "fe29_sqr": [(1,), (2,), (2.79,)],
    "fe29_mul_add_mul": [(2, 2, 1, 3.8), (1, 3.8, 2, 2), (2, 1, 1, 2), (1, 3, 2, 1), (3, 2, 1, 1), (1.9, 2, 2, 2), (1, 3.9, 3.9, 1)],
    "fe29_mul_add_sqr": [(2, 2, 1), (1, 3.8, 2), (2, 2.9, 1.4), (1, 1, 2.6)],
    "fe29_mul_plus": [(2, 3.9, 7.9), (1, 7.8, 7.9), (2.79, 2.79, 7.9), (1, 1, 1)],
    "fe29_sqr_plus": [(2.79, 7.9), (2, 3), (1, 7.9)],
}


def budget_units(name, ws):
    names = FORMS[name][0]
    w = dict(zip(names, ws))
    if name in ("fe29_mul", "fe29_mul_plus"):
        return w["A"] * w["B"]
    if name in ("fe29_sqr", "fe29_sqr_plus"):
        return w["A"] ** 2
    if name == "fe29_mul_add_mul":
        return w["A"] * w["B"] + w["C"] * w["D"]
    return w["A"] * w["B"] + w["C"] ** 2


def test_budgets_are_the_stated_rule():
    for name, cases in BUDGETS.items():
        assert name in FUNCS
        for ws in cases:
            assert budget_units(name, ws) <= 7.8 + 1e-9, (name, ws)
        assert max(budget_units(name, ws) for ws in cases) > 7.7, name     # the rule's edge is among the cases


def rand_lazy(rng, units, extremal):
    hi = units_bound(units)
    if extremal:
        return [h if rng.random() < 0.7 else rng.randrange(h + 1) for h in hi]
    return [rng.randrange(h + 1) for h in hi]


def run_exact(name, limbs, digits=None):
    names, f = FORMS[name]
    r = F.run(FUNCS[name], dict(zip(names, limbs)), digits=digits)
    F.check_result(r, f(*[value(x) for x in limbs]))
    return r


@pytest.mark.parametrize("name", sorted(FORMS))
def test_random_lazy_operands(name):
    """(a) random lazy operands anywhere up to their units, and with most limbs at the bound; every upper column is seen
    with bits 29..31 of its digit all set (the digits the 29-bit schedule never had)."""
    rng = random.Random(len(name) * 1000 + 32)
    top = [0] * (L - 1)
    for ws in BUDGETS[name]:
        for it in range(60):
            digits = []
            run_exact(name, [rand_lazy(rng, w, it % 2 == 0) for w in ws], digits)
            assert len(digits) == L - 1
            for k, u in enumerate(digits):
                top[k] += (u >> W) == 7
    assert all(top), top


@pytest.mark.parametrize("name", sorted(FORMS))
def test_extremal_operands(name):
    """(a) every limb at its bound, for every budget; 0, 1, p - 1, p and 2p in their lazy forms in every position"""
    for ws in BUDGETS[name]:
        run_exact(name, [units_bound(w) for w in ws])
    specials = [[0] * L, [1] + [0] * (L - 1), F.from_int(P - 1), list(P_LIMBS), [2 * x for x in P_LIMBS],
                units_bound(1), [M] * 8 + [M8]]
    n = len(FORMS[name][0])
    rng = random.Random(5)
    for s in specials:
        for t in specials:
            ops = [s, t] + [rng.choice(specials) for _ in range(n - 2)]
            run_exact(name, ops[:n])
            run_exact(name, ops[:n][::-1])


@pytest.mark.parametrize("name", sorted(FORMS))
def test_interval_pass(name):
    """(b) the same statements on upper bounds: no accumulator reaches 2^64, no carry 2^35, the result has 1 unit with
    limb 2 at most 2^12 above (the assertions are the model's; the result's are check_result's)."""
    for ws in BUDGETS[name]:
        digits = []
        r = F.run(FUNCS[name], dict(zip(FORMS[name][0], [units_bound(w) for w in ws])), bound=True, digits=digits)
        F.check_result(r, None)
        assert all(u < U32 for u in digits)
    # the digit itself may be any 32-bit value: the lower columns are bounded with u = 2^32 - 1 whenever the sum can be
    if budget_units(name, BUDGETS[name][0]) >= 1:
        assert max(digits) == U32 - 1


def test_tail_alone():
    """the tail on its widest inputs: digits at their masks, the carries as large as the interval pass lets them be"""
    rng = random.Random(16)
    for _ in range(2000):
        t = [rng.choice([0, 1, M, rng.randrange(M + 1)]) for _ in range(L)]
        c = rng.choice([0, 1, (1 << 41) - 1, rng.randrange(1 << 41)])
        h = rng.choice([0, 1, (1 << 19) - 1, rng.randrange(1 << 19)])
        r = F.mul_tail(t, c, h)
        F.check_result(r, value(t[:8]) + ((t[8] + c) << (W * 8)) + (h << (W * 16 + 32)))
    F.check_result(F.mul_tail([M] * L, (1 << 41) - 1, (1 << 19) - 1, bound=True), None)


def test_model_rejects_an_overflow():
    """(c) past the stated rule the same model reports the overflow: 8 products of limbs whose bounds multiply to more
    than 2^61 do not fit a column"""
    for name, ws in [("fe29_mul", (3, 3)), ("fe29_mul", (2.9, 2.9)), ("fe29_sqr", (2.9,)), ("fe29_mul_add_mul", (2, 2, 2, 2.2)),
                     ("fe29_mul_add_sqr", (2, 2, 2.1)), ("fe29_mul_plus", (3, 3, 1)), ("fe29_sqr_plus", (3, 1))]:
        assert budget_units(name, ws) > 8
        with pytest.raises(AssertionError, match="64-bit accumulator overflow"):
            F.run(FUNCS[name], dict(zip(FORMS[name][0], [units_bound(w) for w in ws])), bound=True)
    with pytest.raises(AssertionError, match="64-bit accumulator overflow"):       # and on integers, not only on bounds
        F.run(FUNCS["fe29_mul"], {"A": units_bound(3), "B": units_bound(3)})
    with pytest.raises(AssertionError):                                              # a carry that leaves limb 2 too wide
        F.check_result(F.mul_tail([M] * L, 0, 1 << 26), None)
    with pytest.raises(AssertionError, match="does not know"):                      # an unknown statement is refused
        F.run(FUNCS["fe29_mul"].replace("u = (uint32_t)d;", "u = (uint32_t)d & F29_M;", 1), {"A": units_bound(1), "B": units_bound(1)})


def test_model_rejects_a_late_read_of_the_old_column():
    """the upper statements keep u and h in d's own registers (d is not an early-clobber operand there): a statement that
    read the digit after d is rewritten would multiply the new column's low register instead"""
    body = FUNCS["fe29_mul"]
    fold, restart = '"v_mad_u64_u32 %1, vcc, %2, %3, %1\\n\\t"', '"v_mad_u64_u32 %0, vcc, %4, 8, 0\\n\\t"'
    at = body.index(fold)
    assert body[at + len(fold):].lstrip().startswith(restart)
    swapped = body[:at] + restart + "\n      " + fold + body[body.index(restart, at) + len(restart):]
    F.run(body, {"A": units_bound(1), "B": units_bound(1)})
    with pytest.raises(AssertionError, match="read after d is written"):
        F.run(swapped, {"A": units_bound(1), "B": units_bound(1)})


def test_header_is_what_the_generator_emits():
    """(d) byte for byte"""
    out = subprocess.run([sys.executable, os.path.join(F.ROOT, "tools", "gen_fe29_mul.py")], check=True, capture_output=True,
                         cwd=os.path.join(F.ROOT, "tools")).stdout
    with open(F.HEADER, "rb") as f:
        assert out == f.read()
