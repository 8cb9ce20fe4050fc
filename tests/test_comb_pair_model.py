"""Model of the comb ladder's column (jacobian29.h: coz29_pair_sum, jpt29_rescale; verify_fast.h: the COMB block of
k_verify_fast), without a GPU.  A column adds the round's two table entries to each other first - E1 of the first half
scalar, phi(E2) of the second, affine over one Z - and their sum to the accumulator: 15 M + 5 S instead of the 16 M + 6 S
of two mixed additions.

  * integers (the limb schedule of test_fe29_model.py): the column is acc + s1 E1 + s2 phi(E2) for points of secp256k1
    brought onto a common Z != 1, all four sign pairs, acc with Z != 1; 19 columns with 18 doublings against pyref; the
    exceptional inputs (E1 = +-E2', acc = +-T, acc.z = 0) give Z3 = 0, and Z3 = 0 survives a column and a doubling;
  * intervals in the units of fe29.h: entries x [1], y [1] out of the table (E2's through fe29_cond_negate1: [<= 2]), the
    accumulator at its invariant x [1], y [<= 2], z [1]; the invariant is closed under column + doubling and
    jpt29_add_affine is called within the operand bounds of its own model row (test_fe29_formulas_model.GUARDED);
  * drift guard against the C++ bodies, one-token mutations the bounds must reject, the product count, and the lazy
    budgets of S2K_HP_JADD_PAIR (ops.hip) that tests/test_gpu_comb_pair.py runs at.
"""
import functools
import itertools
import random
import re

import pytest

import pyref as R
import test_comb_model as cm
import test_fe29_formulas_model as fm
import test_fe29_model as m
from test_fe29_formulas_model import COORD, TWO_P, Y2, cond_negate1, le, within
from test_fe29_model import P, add, cpp, mul, mul_add_mul, negate, normalize_weak, sqr, sqr_plus

N = R.N
JPT_BOX = (COORD, Y2, COORD)
H3 = add.body(fm.PROD, negate.body(fm.PROD, 1))   # h^3 = C - B as the pair sum leaves it: [1] + [2], a product's limb 2 a little above


# ==== the model: intervals ================================================================================================
@cpp("coz29_pair_sum")
def pair_sum(x1, y1, x2, y2):
    h = normalize_weak(add(x2, negate(x1, 1)))
    hh = sqr(h)
    b = mul(x1, hh)
    c = mul(x2, hh)
    nb = negate(b, 1)
    hhh = add(c, nb)
    dy = normalize_weak(add(y2, negate(y1, 1)))
    x = sqr_plus(dy, negate(add(b, c), 2))
    ny = mul_add_mul(dy, add(x, nb), y1, hhh)
    return x, ny, h, hh, hhh


@cpp("jpt29_rescale")
def rescale(p, zz, zzz):
    return (mul(p[0], zz), mul(p[1], zzz), p[2])


def jadd(p, bx, by):
    """m.jpt_add_affine behind a check that it is called as its own model row is: x [1], y [<= 2], z [1]; bx [1], by [<= 2]"""
    row = [g for g in fm.GUARDED if g[3] == "jpt29_add_affine"][0][1]
    assert within(tuple(p) + (bx, by), row), "jpt29_add_affine outside the operand bounds its model row states"
    return m.jpt_add_affine(*p, bx, by)[:3]


def column(acc, x1, y1, x2, y2):
    """the COMB block's column, the calls in the text's order (the lookups and the digit arithmetic are not field calls)"""
    t = pair_sum(x1, y1, x2, cond_negate1(y2))
    acc = rescale(acc, t[3], t[4])
    acc = jadd(acc, t[0], cond_negate1(t[1]))
    return (acc[0], acc[1], mul(acc[2], t[2]))


def comb_block(acc_y, x1, y1, x2, y2, w):
    """the whole block as calls_in reads it: the lead point, the column, the doubling, W"""
    acc = (x1, cond_negate1(acc_y), fm.one())
    acc = column(acc, x1, y1, x2, y2)
    acc = m.jpt_double(*acc)
    return acc[0], acc[1], mul(acc[2], w)


def test_column_and_doubling_keep_the_invariant():
    acc = column(JPT_BOX, COORD, COORD, COORD, COORD)
    assert within(acc, JPT_BOX) and le(acc[1], COORD)              # y leaves the addition at one unit
    d = m.jpt_double(*acc)
    assert within(d, JPT_BOX)
    assert within(column(d, COORD, COORD, COORD, COORD), JPT_BOX)  # ... and the next round takes the doubling's y [<= 2]
    x, ny, h, hh, hhh = pair_sum(COORD, COORD, COORD, Y2)
    assert all(le(v, COORD) for v in (x, ny, h, hh)) and le(hhh, H3)
    assert within(comb_block(COORD, COORD, COORD, COORD, COORD, COORD), JPT_BOX)


def test_contract_of_the_entries():
    """x one unit, y1 one unit, y2 up to two (cond_negate1's 2p - y); more is rejected"""
    pair_sum(COORD, COORD, COORD, TWO_P)
    with pytest.raises(AssertionError):
        pair_sum(COORD, Y2, COORD, Y2)              # y1 of two units: negate(y1, 1), and 9 units in Y_T's reduction
    with pytest.raises(AssertionError):
        pair_sum(m.B.units(2.5), COORD, COORD, Y2)  # negate(x1, 1)
    with pytest.raises(AssertionError):
        column(JPT_BOX, COORD, COORD, COORD, m.B.units(2.01))      # cond_negate1 takes at most 2p


def test_the_model_counts_20_products():
    def products(fn, *args):
        """(field products, reductions) of one run of the model: every product goes through m.mulsum, once per reduction"""
        seen, orig = [], m.mulsum

        def counting(pairs, addend=None):
            seen.append(len(pairs))
            return orig(pairs, addend)
        m.mulsum = counting
        try:
            fn(*args)
        finally:
            m.mulsum = orig
        return sum(seen), len(seen)

    assert products(pair_sum.body, COORD, COORD, COORD, Y2) == (6, 5)           # 4 M + 2 S in five reductions
    assert products(rescale.body, JPT_BOX, COORD, H3) == (2, 2)
    assert products(m.jpt_add_affine.body, *JPT_BOX, COORD, Y2) == (11, 10)
    assert products(column, JPT_BOX, COORD, COORD, COORD, COORD) == (20, 18)   # two mixed additions: (22, 20)
    assert 19 * 20 + 18 * 7 == 506 and 19 * 22 + 18 * 7 == 544                  # the ladder; 526 / 564 with what stands around it


# ==== the model: integers ================================================================================================
def _add(a, b):
    r = [x + y for x, y in zip(a, b)]
    assert all(x < m.U32 for x in r)
    return r


def cond_negate1_int(a, neg):
    if not neg:
        return list(a)
    assert all(x <= 2 * p for x, p in zip(a, m.P_LIMBS))
    return [2 * p - x for x, p in zip(a, m.P_LIMBS)]


def pair_sum_int(x1, y1, x2, y2):
    h = m.normalize_weak_int(_add(x2, m.negate_int(x1, 1)))
    hh = m.mulsum_int([(h, h)])
    b = m.mulsum_int([(x1, hh)])
    c = m.mulsum_int([(x2, hh)])
    nb = m.negate_int(b, 1)
    hhh = _add(c, nb)
    dy = m.normalize_weak_int(_add(y2, m.negate_int(y1, 1)))
    x = m.mulsum_int([(dy, dy)], m.negate_int(_add(b, c), 2))
    ny = m.mulsum_int([(dy, _add(x, nb)), (y1, hhh)])
    return x, ny, h, hh, hhh


def add_affine_int(p, bx, by):
    x, y, z = p
    zz = m.mulsum_int([(z, z)])
    nx = m.negate_int(x, 1)
    h = m.mulsum_int([(bx, zz)], nx)
    ns = m.negate_int(m.mulsum_int([(by, zz)]), 1)
    i = m.mulsum_int([(ns, z)], y)
    z3 = m.mulsum_int([(z, h)])
    h2 = m.mulsum_int([(h, h)])
    h3 = m.mulsum_int([(h2, m.negate_int(h, 1))])
    t = m.mulsum_int([(nx, h2)])
    x3 = m.mulsum_int([(i, i)], _add(_add(h3, t), t))
    t = _add(t, x3)
    return x3, m.mulsum_int([(t, i), (h3, y)]), z3


def double_int(p):
    x, y, z = p
    z3 = m.mulsum_int([(y, z)])
    s = m.mulsum_int([(y, y)])
    l = m.half_int([3 * v for v in m.mulsum_int([(x, x)])])
    t = m.mulsum_int([(m.negate_int(s, 1), x)])
    x3 = m.mulsum_int([(l, l)], _add(t, t))
    t = _add(t, x3)
    return x3, m.negate_int(m.mulsum_int([(t, l), (s, s)]), 1), z3


def column_int(acc, e1, e2, n1, n2):
    """the column as the kernel runs it: E2 with its sign relative to E1's, the sum negated once"""
    t = pair_sum_int(e1[0], e1[1], e2[0], cond_negate1_int(e2[1], n1 != n2))
    acc = (m.mulsum_int([(acc[0], t[3])]), m.mulsum_int([(acc[1], t[4])]), acc[2])
    acc = add_affine_int(acc, t[0], cond_negate1_int(t[1], not n1))
    return acc[0], acc[1], m.mulsum_int([(acc[2], t[2])])


def _lift(pt, z):
    return (m.from_int(pt[0] * z * z % P), m.from_int(pt[1] * pow(z, 3, P) % P))


def _aff(acc, w):
    z = m.value(acc[2]) * w % P
    if z == 0:
        return None
    return cm._affine(m.value(acc[0]), m.value(acc[1]), z)


def _phi(pt):
    return (pt[0] * R.BETA % P, pt[1])


def _signed(pt, neg):
    return R.neg(pt) if neg else pt


def test_column_is_acc_plus_both_entries():
    rng = random.Random(1820)
    for it in range(24):
        n1, n2 = bool(it & 1), bool(it & 2)
        A, E1, E2 = (R.mul(rng.randrange(1, N), R.G) for _ in range(3))
        w = rng.randrange(2, P)                                    # the table's common Z
        za = rng.randrange(2, P) if it >= 4 else 1                 # the accumulator's own
        ax, ay = _lift(A, w * za % P)
        acc = (ax, ay, m.from_int(za))
        got = column_int(acc, _lift(E1, w), _lift(_phi(E2), w), n1, n2)
        want = R.add(R.add(A, _signed(E1, n1)), _signed(_phi(E2), n2))
        assert _aff(got, w) == want, it
        assert all(x <= m.M + (1 << 20) for v in got for x in v)


def test_nineteen_columns_with_doublings_against_pyref():
    """the ladder's own sequence on the limb schedule: the lead, 19 rounds, W - for a table built on values"""
    import test_glv_odd_model as glv
    rng = random.Random(1821)
    d = rng.randrange(1, N)
    Q = R.mul(d, R.G)
    lead, pt, zac = cm.chain_comb(Q)
    entries, (ls, ld), W = cm.finish_comb(lead, pt, zac)
    for u2 in (3, R.LAMBDA + 1, rng.randrange(1, N)):
        k1, k2 = glv.make_odd(*glv.split_reference(u2))
        neg1, neg2 = k1 < 0, k2 < 0
        lx, ly = ls if neg1 == neg2 else ld
        acc = (m.from_int(lx), cond_negate1_int(m.from_int(ly), neg1), m.from_int(1))
        d1, d2 = cm.comb_digits(abs(k1)), cm.comb_digits(abs(k2))
        for r in range(cm.SPACING):
            if r:
                acc = double_int(acc)
            (i1, m1), (i2, m2) = d1[r], d2[r]
            e1, e2 = entries[i1], entries[i2]
            acc = column_int(acc, (m.from_int(e1[0]), m.from_int(e1[1])), (m.from_int(e2[2]), m.from_int(e2[1])), neg1 != m1, neg2 != m2)
            assert all(x <= 2 * m.M + (1 << 21) for v in acc for x in v)
        assert _aff(acc, W) == R.mul(u2, Q), hex(u2)


def test_exceptional_inputs_give_z_zero_and_it_stays():
    rng = random.Random(1822)
    w = rng.randrange(2, P)
    A, E1, E2 = (R.mul(rng.randrange(1, N), R.G) for _ in range(3))
    za = rng.randrange(2, P)
    acc = _lift(A, w * za % P) + (m.from_int(za),)
    e1, e2 = _lift(E1, w), _lift(E2, w)
    zero = lambda r: m.value(r[2]) % P == 0
    cases = []
    # E1 = E2' and E1 = -E2': h = 0
    cases.append(column_int(acc, e1, e1, False, False))
    cases.append(column_int(acc, e1, (e1[0], m.from_int(-m.value(e1[1]) % P)), False, False))
    cases.append(column_int(acc, e1, e1, False, True))
    # acc = +-T for T = s1 E1 + s2 E2
    for n1, n2 in ((False, False), (True, False)):
        T = R.add(_signed(E1, n1), _signed(E2, n2))
        for sign in (False, True):
            at = _lift(_signed(T, sign), w * za % P) + (m.from_int(za),)
            cases.append(column_int(at, e1, e2, n1, n2))
    # acc.z = 0
    cases.append(column_int((acc[0], acc[1], m.from_int(0)), e1, e2, False, True))
    for k, r in enumerate(cases):
        assert zero(r), k
        nxt = column_int(r, e2, e1, True, False)
        assert zero(nxt) and zero(double_int(nxt)) and zero(column_int(double_int(r), e1, e2, False, False)), k
    assert not zero(column_int(acc, e1, e2, False, False))


def test_column_on_extremal_limbs():
    """every limb of every operand at the invariant's bound: the formulas as polynomials"""
    rng = random.Random(1823)
    for it in range(100):
        ext = it % 2 == 0
        acc = (m.rand_lazy(rng, 1, ext), m.rand_lazy(rng, 2, ext), m.rand_lazy(rng, 1, it % 3 == 0))
        x1, y1, x2, y2 = (m.rand_lazy(rng, 1, ext if k != 2 else it % 3 == 0) for k in range(4))
        n1, n2 = bool(it & 4), bool(it & 8)
        X, Y, Z, a1, b1, a2, b2 = (m.value(v) % P for v in acc + (x1, y1, x2, y2))
        b2 = -b2 % P if n1 != n2 else b2
        h = (a2 - a1) % P
        A_, B_, C_ = h * h % P, a1 * h * h % P, a2 * h * h % P
        xt = ((b2 - b1) ** 2 - B_ - C_) % P
        yt = ((b2 - b1) * (B_ - xt) - b1 * (C_ - B_)) % P
        yt = -yt % P if n1 else yt
        Xs, Ys = X * A_ % P, Y * (C_ - B_) % P
        H = (xt * Z * Z - Xs) % P
        I = (Ys - yt * Z ** 3) % P
        x3 = (I * I - H ** 3 - 2 * Xs * H * H) % P
        y3 = (I * (x3 - Xs * H * H) - Ys * H ** 3) % P
        got = column_int(acc, (x1, y1), (x2, y2), n1, n2)
        assert [m.value(v) % P for v in got] == [x3, y3, Z * H * h % P], it


# ==== drift guard and mutations ============================================================================================
def comb_block_text():
    body = fm.body_of("verify_fast.h", "k_verify_fast")
    return body[body.index("if constexpr (COMB) {"):body.index("} else if constexpr (KEYED) {")]


GUARDED = [
    (pair_sum, (COORD, COORD, COORD, Y2), "jacobian29.h", "coz29_pair_sum"),
    (rescale, (JPT_BOX, COORD, H3), "jacobian29.h", "jpt29_rescale"),
]


@pytest.mark.parametrize("g", GUARDED, ids=[g[3] for g in GUARDED])
def test_drift_guard(g, tracked):
    fn, args, fname, func = g
    assert m.record(fn, *args) == fm.calls_in(fm.body_of(fname, func)), f"{func} ({fname}) no longer matches its model"


@pytest.fixture
def tracked(monkeypatch):
    monkeypatch.setattr(fm, "TRACKED", re.compile(fm.TRACKED.pattern.replace(r"(fe29_\w+", r"(fe29_\w+|coz29_\w+")))


def test_drift_guard_of_the_comb_block(tracked):
    """the block's tracked calls, in order, are the model's: the lead point, ONE column, the doubling, W"""
    got = fm.calls_in(comb_block_text())

    def block(*a):
        # the model's top-level calls: column() and jadd() are plain functions, so what they call is recorded at depth 0
        return comb_block(*a)
    assert m.record(block, COORD, COORD, COORD, COORD, COORD, COORD) == got
    text = comb_block_text()
    assert text.count("coz29_pair_sum(") == 1 and text.count("jpt29_rescale(") == 1 and text.count("ke_load_xy(") == 3
    assert "coz29_pair_sum(x1, y1, x2, fe29_cond_negate1(y2, n1 != n2))" in text          # E2 with its sign relative to E1's
    assert "jpt29_add_affine(acc, t.x, fe29_cond_negate1(t.ny, !n1))" in text             # ny = -Y_T: negated unless E1 is negative
    # the operation this block does not get: the same text in ops.hip's k_pair_op (S2K_HP_JADD_PAIR), which the device test runs
    ops = fm.body_of("ops.hip", "k_pair_op")
    for line in ("coz29_pair_sum(x1, y1, x2, fe29_cond_negate1(y2, n1 != n2))", "acc = jpt29_rescale(acc, t.hh, t.hhh);",
                 "acc = jpt29_add_affine(acc, t.x, fe29_cond_negate1(t.ny, !n1));", "acc.z = fe29_mul(acc.z, t.h);"):
        assert line in ops and line in text, line


PS_ARGS = (COORD, COORD, COORD, Y2)
MUTATIONS = [
    ("coz29_pair_sum: fe29_negate(x1, 1) -> 0", pair_sum, PS_ARGS, ("fe29_negate", 0, fm._lower)),
    ("coz29_pair_sum: drop fe29_normalize_weak of h", pair_sum, PS_ARGS, ("fe29_normalize_weak", 0, None)),
    ("coz29_pair_sum: fe29_negate(b, 1) -> 0", pair_sum, PS_ARGS, ("fe29_negate", 1, fm._lower)),
    ("coz29_pair_sum: fe29_negate(y1, 1) -> 0", pair_sum, PS_ARGS, ("fe29_negate", 2, fm._lower)),
    ("coz29_pair_sum: drop fe29_normalize_weak of y2 - y1", pair_sum, PS_ARGS, ("fe29_normalize_weak", 1, None)),
    ("coz29_pair_sum: fe29_negate(fe29_add(b, c), 2) -> 1", pair_sum, PS_ARGS, ("fe29_negate", 3, fm._lower)),
]


@pytest.mark.parametrize("mu", MUTATIONS, ids=[mu[0] for mu in MUTATIONS])
def test_mutation_is_rejected(mu):
    _, fn, args, mutation = mu
    fn(*args)
    with pytest.raises(AssertionError):
        m.mutated(fn, mutation, *args)


# ==== lazy budgets of S2K_HP_JADD_PAIR (ops.hip: k_pair_op without the lift) ================================================
def _pair_nolift(c):
    """operands 0, 1 (P), 3, 4 (E1), 5, 6 (E2) in their lazy forms, P = (a, b, 1); one column, and a column behind a doubling"""
    px, py, x1, y1, x2, y2 = map(fm.lazy_bound, c)
    acc = column((px, py, fm.one.body()), x1, y1, x2, y2)
    column(m.jpt_double(*acc), x1, y1, x2, y2)


@functools.lru_cache(maxsize=None)
def pair_budgets():
    ok = {t for t in itertools.product(fm.CODES, repeat=6) if fm._accepts(_pair_nolift, t)}
    return sorted(t for t in ok if not any(t[:i] + (u,) + t[i + 1:] in ok for i in range(6) for u in fm._above(t[i])))


# pinned: a model change that moves them has to move these too.  P's x and E2's x meet products only (h is weakly
# normalised, x2's other use is x2 h^2) and take everything; P's y takes the accumulator's two units (one multiple of p, or
# the borrow spread); x1, y1 and y2 are taken at one unit (fe29_negate(., 1), fe29_cond_negate1).
EXPECTED_PAIR_BUDGETS = [(7, 1, 0, 0, 7, 0), (7, 4, 0, 0, 7, 0)]


def test_pair_lazy_budgets():
    tops = pair_budgets()
    assert tops == EXPECTED_PAIR_BUDGETS
    for t in tops:
        for i in range(6):
            for u in fm._above(t[i]):
                assert not fm._accepts(_pair_nolift, t[:i] + (u,) + t[i + 1:])


# ==== the scalars of the device test's ECDSA call ===========================================================================
def paired_u2(rng, count):
    """u2 = k (1 + lambda) and k (1 - lambda) for odd k < 2^127: the split halves are (k, k) and (k, -k), so every column of
    the comb reads the same entry index in both halves - x2 = beta x1, in both relative signs"""
    out = []
    for i in range(count):
        k = rng.randrange(1 << 126) * 2 + 1
        out.append(k * (1 + R.LAMBDA) % N if i % 2 == 0 else k * (1 - R.LAMBDA) % N)
    return out


def test_paired_u2_split_into_equal_halves():
    """what tests/test_gpu_comb_pair.py's ECDSA call relies on: the device's split (its model) gives |k1| = |k2|, with both relative signs"""
    rel = set()
    import test_glv_odd_model as glv
    for u2 in paired_u2(random.Random(1860), 64):
        k1, k2 = glv.make_odd(*glv.split_reference(u2))
        assert abs(k1) == abs(k2) and k1 & 1
        rel.add((k1 < 0) == (k2 < 0))
    assert rel == {True, False}
