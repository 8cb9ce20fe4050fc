"""Model of the two formulas the one-pass table build adds, on the interval and integer layers of test_fe29_model.py
and test_fe29_formulas_model.py:

  * coz29_add_update (keyed.hip): Meloni's co-Z addition with update, the odd multiples of k_key_finish;
  * xyzz29_add_affine_first (xyzz29.h): affine + affine to XYZZ, the first addition of k_generator_part;
  * k_key_finish itself: its calls against the C++ body (drift guard), its bounds, and its VALUES for one key - the
    chains of the eight lanes, the prefix / suffix products across them, the scaling walk - against tests/pyref.py.

Units (fe29.h): a product needs the products of its operands' units, summed over the fused terms, <= 7.8; the interval
layer carries the limbs' upper bounds through the exact call sequence and asserts every 32- and 64-bit width.
"""
import random

import pytest

import pyref as R
import test_fe29_formulas_model as fm
import test_fe29_model as m
from test_fe29_formulas_model import CANON, COORD, NW, PROD, TWO_P, XYZZ_INV, Y2, from_words, group_shl, le, one, select, within, \
    xyzz_add_affine, zero
from test_fe29_model import B, P, add, cpp, mul, mul_add_mul, mul_plus, negate, normalize_weak, sqr, sqr_plus

BETA = R.BETA


# ---- interval models ----------------------------------------------------------------------------------------------------
@cpp("coz29_add_update")
def coz_add_update(s):
    px, py, qx, qy = s
    h = normalize_weak(add(qx, negate(px, 1)))
    a = sqr(h)
    b = mul(px, a)
    c = mul(qx, a)
    dy = normalize_weak(add(qy, negate(py, 1)))
    xr = sqr_plus(dy, negate(add(b, c), 2))
    e = mul(py, add(c, negate(b, 1)))
    yr = mul_plus(dy, add(b, negate(xr, 1)), negate(e, 1))
    return (b, e, xr, yr), h


@cpp("xyzz29_add_affine_first")
def xyzz_add_affine_first(ax, ay, bx, by):
    nx = negate(ax, 1)
    pp_ = normalize_weak(add(bx, nx))
    rn = normalize_weak(add(ay, negate(by, 2)))
    pp = sqr(pp_)
    ppp = mul(pp, pp_)
    pppn = negate(ppp, 1)
    qn = mul(nx, pp)
    rx = sqr_plus(rn, add(add(pppn, qn), qn))
    t = add(qn, rx)
    ry = mul_add_mul(t, rn, pppn, ay)
    return (rx, ry, pp, ppp)


@cpp("fe29_group_shr")
def group_shr(a):
    return fm.join(a, one.body())


@cpp("k_key_finish")
def key_finish(ex, ey, ezb, lead):
    """one lane: the base entry as k_key_chain stores it (x [1], y [<= 2], z [1]), every loop's body once; lead: the lead
    pair's x, y, z, x, y as k_key_chain stores them.  Returns everything the kernel stores."""
    lx, ly, lz, dx, dy = lead
    a0 = (ex, ey, one())
    d = m.jpt_double(*a0)
    c2 = sqr(d[2])
    c3 = mul(c2, d[2])
    s = (d[0], d[1], mul(a0[0], c2), mul(a0[1], c3))
    zt = mul(d[2], ezb)
    outs = [s[2], s[3]]
    s, h = coz_add_update(s)
    outs += [s[2], s[3], h]
    zt = mul(zt, h)
    pre = select(group_shr(zt), lz)
    pre = mul(pre, group_shr(pre))
    pre = mul(pre, group_shr(pre))
    pre = mul(pre, group_shr(pre))
    suf = group_shl(zt)
    suf = mul(suf, group_shl(suf))
    suf = mul(suf, group_shl(suf))
    suf = mul(suf, group_shl(suf))
    rr = mul(pre, suf)
    co = mul(suf, zt)
    beta = from_words()
    q2 = sqr(rr)
    q3 = mul(q2, rr)
    x = mul(s[2], q2)
    y = mul(s[3], q3)
    outs += [x, y, mul(x, beta)]
    rr = mul(rr, h)
    outs.append(mul(co, lz))
    s2 = sqr(co)
    s3 = mul(s2, co)
    outs += [mul(lx, s2), mul(ly, s3), zero(), mul(dx, s2), mul(dy, s3), zero()]
    return s, zt, rr, outs


COZ_INV = (COORD,) * 4                    # a coz29: all four coordinates [1]
LEAD = (NW, PROD, PROD, NW, PROD)         # k_key_chain's lead pair (test_fe29_formulas_model.key_chain)


# ==== bounds and closure ================================================================================================
def test_coz_step_invariant_closed():
    s, h = coz_add_update(COZ_INV)
    assert within(s, COZ_INV) and le(h, COORD)
    for _ in range(7):                    # chained, as k_key_finish chains it
        s, h = coz_add_update(s)
        assert within(s, COZ_INV) and le(h, COORD)
    # the first step takes D.y as jpt29_double leaves it (2p - a product limb by limb), nothing larger
    s, h = coz_add_update((COORD, TWO_P, COORD, COORD))
    assert within(s, COZ_INV) and le(h, COORD)
    with pytest.raises(AssertionError):
        coz_add_update((COORD, Y2, COORD, COORD))


def test_affine_first_bounds():
    # k_generator_part: both points from words; the ops form: x [1], y up to 2p limb by limb
    for ax, ay, bx, by in ((CANON,) * 4, (COORD, TWO_P, COORD, TWO_P), (COORD, Y2, COORD, NW)):
        r = xyzz_add_affine_first(ax, ay, bx, by)
        assert within(r, XYZZ_INV), [v.hi for v in r]
        assert within(xyzz_add_affine(r, CANON, CANON), XYZZ_INV)      # what the loop of k_generator_part does next
    with pytest.raises(AssertionError):
        xyzz_add_affine_first(COORD, B.units(3), COORD, COORD)          # mul_add_mul: [2]*[1] + [2]*[3] > 7.8
    with pytest.raises(AssertionError):
        xyzz_add_affine_first(COORD, COORD, COORD, B.units(3.1))        # negate(by, 2)


def test_key_finish_bounds():
    s, zt, rr, outs = key_finish(COORD, Y2, COORD, LEAD)
    assert within(s, COZ_INV) and le(zt, COORD) and le(rr, COORD)
    assert all(le(o, COORD) for o in outs), "a stored value is above 1 unit"
    # the running products fed back in (the loops' later trips)
    s2, h = coz_add_update(s)
    assert within(s2, COZ_INV) and le(mul(zt, h), COORD) and le(mul(rr, h), COORD)


# ==== drift guard and non-vacuity ========================================================================================
@pytest.fixture
def tracked(monkeypatch):
    monkeypatch.setattr(fm, "TRACKED", __import__("re").compile(fm.TRACKED.pattern.replace(r"(fe29_\w+", r"(fe29_\w+|coz29_\w+")))


GUARDED = [
    (coz_add_update, (COZ_INV,), "keyed.hip", "coz29_add_update"),
    (group_shr, (COORD,), "keyed.hip", "fe29_group_shr"),
    (key_finish, (COORD, Y2, COORD, LEAD), "keyed.hip", "k_key_finish"),
    (xyzz_add_affine_first, (COORD, Y2, COORD, Y2), "xyzz29.h", "xyzz29_add_affine_first"),
]


@pytest.mark.parametrize("g", GUARDED, ids=[g[3] for g in GUARDED])
def test_drift_guard(g, tracked):
    fn, args, fname, func = g
    assert m.record(fn, *args) == fm.calls_in(fm.body_of(fname, func)), f"{func} ({fname}) no longer matches its model"


def test_generator_part_uses_the_first_addition_once():
    body = fm.body_of("lane_kernels.hip", "k_generator_part")
    assert body.count("xyzz29_add_affine_first(") == 1 and body.count("xyzz29_add_affine(") == 1


MUTATIONS = [
    ("coz29_add_update: fe29_negate(s.px, 1) -> 0", coz_add_update, (COZ_INV,), ("fe29_negate", 0, fm._lower)),
    ("coz29_add_update: drop fe29_normalize_weak of h", coz_add_update, (COZ_INV,), ("fe29_normalize_weak", 0, None)),
    ("coz29_add_update: drop fe29_normalize_weak of Y_Q - Y_P", coz_add_update, (COZ_INV,), ("fe29_normalize_weak", 1, None)),
    ("coz29_add_update: fe29_negate(fe29_add(b, c), 2) -> 1", coz_add_update, (COZ_INV,), ("fe29_negate", 2, fm._lower)),
    ("coz29_add_update: fe29_negate(e, 1) -> 0", coz_add_update, (COZ_INV,), ("fe29_negate", 5, fm._lower)),
    ("xyzz29_add_affine_first: drop fe29_normalize_weak of P", xyzz_add_affine_first, (COORD, Y2, COORD, Y2),
     ("fe29_normalize_weak", 0, None)),
    ("xyzz29_add_affine_first: fe29_negate(by, 2) -> 1", xyzz_add_affine_first, (COORD, Y2, COORD, B.units(2.5)),
     ("fe29_negate", 1, fm._lower)),
    ("xyzz29_add_affine_first: fe29_negate(ppp, 1) -> 0", xyzz_add_affine_first, (COORD, Y2, COORD, Y2), ("fe29_negate", 2, fm._lower)),
    ("k_key_finish: jpt29_double's fe29_negate(s, 1) -> 0", key_finish, (COORD, Y2, COORD, LEAD), ("fe29_negate", 0, fm._lower, True)),
]


@pytest.mark.parametrize("mu", MUTATIONS, ids=[mu[0] for mu in MUTATIONS])
def test_mutation_is_rejected(mu):
    _, fn, args, mutation = mu
    fn(*args)                                        # the unmutated model passes on the same inputs
    with pytest.raises(AssertionError):
        m.mutated(fn, mutation, *args)


# ==== integers: the schedule limb by limb ================================================================================
def _add(a, b):
    r = [x + y for x, y in zip(a, b)]
    assert all(x < m.U32 for x in r)
    return r


def coz_step_int(s):
    px, py, qx, qy = s
    h = m.normalize_weak_int(_add(qx, m.negate_int(px, 1)))
    a = m.mulsum_int([(h, h)])
    b = m.mulsum_int([(px, a)])
    c = m.mulsum_int([(qx, a)])
    dy = m.normalize_weak_int(_add(qy, m.negate_int(py, 1)))
    xr = m.mulsum_int([(dy, dy)], m.negate_int(_add(b, c), 2))
    e = m.mulsum_int([(py, _add(c, m.negate_int(b, 1)))])
    yr = m.mulsum_int([(dy, _add(b, m.negate_int(xr, 1)))], m.negate_int(e, 1))
    return (b, e, xr, yr), h


def affine_first_int(ax, ay, bx, by):
    nx = m.negate_int(ax, 1)
    pp_ = m.normalize_weak_int(_add(bx, nx))
    rn = m.normalize_weak_int(_add(ay, m.negate_int(by, 2)))
    pp = m.mulsum_int([(pp_, pp_)])
    ppp = m.mulsum_int([(pp, pp_)])
    pppn = m.negate_int(ppp, 1)
    qn = m.mulsum_int([(nx, pp)])
    rx = m.mulsum_int([(rn, rn)], _add(_add(pppn, qn), qn))
    t = _add(qn, rx)
    ry = m.mulsum_int([(t, rn), (pppn, ay)])
    return rx, ry, pp, ppp


def _lazy(rng, v, units):
    """v in a lazy form: a random multiple of p below `units` added, the top limb taking what the low ones leave"""
    k = rng.randrange(int(units)) if units >= 2 else 0
    return m.from_int(v % P + k * P)


def _double_jacobian(x, y):
    """2 (x, y, 1) by jacobian29.h's formulas, on values"""
    half = pow(2, -1, P)
    l = 3 * x * x * half % P
    s = y * y % P
    t = -x * s % P
    x3 = (l * l + 2 * t) % P
    y3 = -(l * (x3 + t) + s * s) % P
    return x3, y3, y % P


def _affine(X, Y, Z):
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def test_seven_chained_steps_give_the_odd_multiples():
    rng = random.Random(2607)
    for it in range(12):
        base = R.mul(rng.randrange(1, R.N), R.G)
        zb = rng.randrange(1, P)                                   # the base as k_key_chain leaves it: Jacobian, any Z
        X, Y = base[0] * zb * zb % P, base[1] * zb ** 3 % P
        dx, dy, dz = _double_jacobian(X, Y)                        # on the curve isomorphic by zb
        py = m.negate_int(m.from_int(-dy % P), 1)                 # D.y as jpt29_double leaves it: 2p - a product
        s = (m.from_int(dx), py, m.from_int(X * dz * dz % P), m.from_int(Y * dz ** 3 % P))
        z = dz * zb % P                                            # Z of both points over secp256k1
        assert _affine(m.value(s[2]), m.value(s[3]), z) == base
        assert _affine(m.value(s[0]), m.value(s[1]), z) == R.mul(2, base)
        for j in range(1, 8):
            s, h = coz_step_int(s)
            z = z * m.value(h) % P                                 # Z_j = Z_(j-1) h_j
            assert _affine(m.value(s[2]), m.value(s[3]), z) == R.mul(2 * j + 1, base), (it, j)
            assert _affine(m.value(s[0]), m.value(s[1]), z) == R.mul(2, base), (it, j)     # the running copy of D
            assert all(x <= m.M + (1 << 20) for x in s[0] + s[1] + s[2] + s[3])


def test_coz_step_on_extremal_limbs():
    """the schedule at the invariant's edge: every limb of every operand at its bound (values are then arbitrary field
    elements, so the formulas are compared as polynomials)"""
    rng = random.Random(11)
    for it in range(200):
        s = tuple(m.rand_lazy(rng, 1, it % 2 == 0) for _ in range(4))
        px, py, qx, qy = (m.value(v) for v in s)
        (b, e, xr, yr), h = coz_step_int(s)
        hv = (qx - px) % P
        A, Bv, C = hv * hv % P, px * hv * hv % P, qx * hv * hv % P
        assert m.value(h) % P == hv and m.value(b) % P == Bv and m.value(e) % P == py * (C - Bv) % P
        X = ((qy - py) ** 2 - Bv - C) % P
        assert m.value(xr) % P == X and m.value(yr) % P == ((qy - py) * (Bv - X) - py * (C - Bv)) % P


def test_affine_first_on_integers():
    rng = random.Random(12)
    for it in range(60):
        a, b = R.mul(rng.randrange(1, R.N), R.G), R.mul(rng.randrange(1, R.N), R.G)
        if it % 4 == 0:
            b = a                                                   # P + P
        if it % 4 == 1:
            b = R.neg(a)                                            # P - P
        ax, bx = m.from_int(a[0]), m.from_int(b[0])
        ay, by = _lazy(rng, a[1], 2 if it % 3 else 1), _lazy(rng, b[1], 2 if it % 5 else 1)
        rx, ry, zz, zzz = (m.value(v) % P for v in affine_first_int(ax, ay, bx, by))
        if a[0] == b[0]:
            assert zz == 0 and zzz == 0                             # the sticky exceptional case
            continue
        assert pow(zz, 3, P) == zzz * zzz % P
        assert (rx * pow(zz, -1, P) % P, ry * pow(zzz, -1, P) % P) == R.add(a, b)


# ==== values: k_key_finish for one key ======================================================================================
def key_finish_values(bases, lead_s, lead_d, lead_z):
    """the kernel's steps on field values; bases[c] = (X, Y, Z) of 2^(16c) Q.  Returns W, entries[c][j] = (x, y, beta x),
    and the two lead entries."""
    zt, cur, hs = [], [], []
    for X, Y, zb in bases:
        dx, dy, dz = _double_jacobian(X, Y)
        s = [dx, dy, X * dz * dz % P, Y * dz ** 3 % P]
        pts, h_c, z = [(s[2], s[3])], [], dz * zb % P
        for _ in range(7):
            px, py, qx, qy = s
            h = (qx - px) % P
            a = h * h % P
            b, c = px * a % P, qx * a % P
            xr = ((qy - py) ** 2 - b - c) % P
            e = py * (c - b) % P
            s = [b, e, xr, ((qy - py) * (b - xr) - e) % P]
            pts.append((s[2], s[3]))
            h_c.append(h)
            z = z * h % P
        zt.append(z)
        cur.append(pts)
        hs.append(h_c)

    def shr(v, n, keep):
        return [v[c - n] if keep(c) else 1 for c in range(8)]

    def shl(v, n, keep):
        return [v[c + n] if keep(c) else 1 for c in range(8)]

    def mulv(a, b):
        return [x * y % P for x, y in zip(a, b)]
    pre = [lead_z if c == 0 else v for c, v in enumerate(shr(zt, 1, lambda c: c > 0))]
    pre = mulv(pre, shr(pre, 1, lambda c: c > 0))
    pre = mulv(pre, shr(pre, 2, lambda c: c > 1))
    pre = mulv(pre, shr(pre, 4, lambda c: c > 3))
    suf = shl(zt, 1, lambda c: c < 7)
    suf = mulv(suf, shl(suf, 1, lambda c: c < 7))
    suf = mulv(suf, shl(suf, 2, lambda c: c < 6))
    suf = mulv(suf, shl(suf, 4, lambda c: c < 4))
    rr = mulv(pre, suf)
    co = suf[0] * zt[0] % P
    W = co * lead_z % P
    leads = [(x * co * co % P, y * co ** 3 % P) for x, y in (lead_s, lead_d)]
    entries = [[None] * 8 for _ in range(8)]
    for c in range(8):
        r = rr[c]
        for j in range(7, -1, -1):
            x, y = cur[c][j]
            x, y = x * r * r % P, y * r ** 3 % P
            entries[c][j] = (x, y, x * BETA % P)
            if j:
                r = r * hs[c][j - 1] % P
    return W, entries, leads


def test_key_finish_values_are_the_table():
    """every entry comes out as (W^2 x, W^3 y, beta W^2 x) of (2j + 1) 2^(16c) Q, the lead pair as L +- phi(L) under the
    same W, for the W the kernel stores"""
    rng = random.Random(41)
    for _ in range(2):
        Q = R.mul(rng.randrange(1, R.N), R.G)
        bases = []
        for c in range(8):
            pt, z = R.mul(1 << (16 * c), Q), rng.randrange(1, P)
            bases.append((pt[0] * z * z % P, pt[1] * z ** 3 % P, z))
        L = R.mul(1 << 116, Q)
        phiL = (L[0] * BETA % P, L[1])
        lz = rng.randrange(1, P)
        jac = lambda pt: (pt[0] * lz * lz % P, pt[1] * lz ** 3 % P)
        W, entries, leads = key_finish_values(bases, jac(R.add(L, phiL)), jac(R.add(L, R.neg(phiL))), lz)
        w2, w3 = W * W % P, pow(W, 3, P)
        for c in range(8):
            for j in range(8):
                x, y = R.mul((2 * j + 1) << (16 * c), Q)
                assert entries[c][j] == (x * w2 % P, y * w3 % P, x * w2 * BETA % P), (c, j)
        for got, pt in zip(leads, (R.add(L, phiL), R.add(L, R.neg(phiL)))):
            assert got == (pt[0] * w2 % P, pt[1] * w3 % P)


# ==== k_generator_part: the first addition never meets equal x ============================================================
def test_generator_windows_never_meet():
    """T_0[d0] = (d0 - S) G with S = sum_{i>=1} 2^(b i), T_1[d1] = (d1 + 1) 2^b G (gtable.hip).  For every window width the
    tables are built with, no pair of digits makes the two points equal or opposite: d0 - S = +-(d1 + 1) 2^b (mod n) has
    no solution with d0, d1 < 2^b, so the ZZ = 0 path of xyzz29_add_affine_first is reached by no u1 (its formula-level
    test runs it through s2k_fp_op_batch_ex instead)."""
    for b in range(8, 27):
        w = (256 + b - 1) // b
        S = sum(1 << (b * i) for i in range(1, w))
        assert w > 3 and S < R.N
        lo, hi = (1 << b), (1 << (2 * b))                       # the range of (d1 + 1) 2^b
        # equal: (d1 + 1) 2^b = d0 - S + n, a value in (n - S, n - S + 2^b)
        assert R.N - S > hi
        # opposite: (d1 + 1) 2^b = S - d0, a value in (S - 2^b, S], below n and above 2^(2b)
        assert S - (1 << b) > hi and lo > 0
