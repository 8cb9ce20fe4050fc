"""Interval model of the lazy 9x29 formulas the multiscalar and key-table kernels run (xyzz29.h, pt29q.h, aff29.h,
msm_piece / msm_point_of of msm.hip, the wide joint-table kernels of keyed.hip), on the interval layer of
test_fe29_model.py.

  * bounds: every formula is run on upper bounds of its operands' limbs at their stated invariants; no 32-bit limb,
    64-bit column sum or negate() bias may overflow, and the invariants are closed under the formulas' own chaining;
  * call sites: every fe29_eq / fe29_is_zero / fe29_normalize / fe29_inv_gcd of verify_fast.h, lane_kernels.hip, worklist.hip,
    small_call.hip, keyed.hip, msm.hip, msm_terms.h and rlc.hip has a row with its modelled operand bound (fe29_normalize_weak's input contract:
    limbs < 2^32 - 2^18);
  * drift guard: the calls each model makes are compared with the calls of the C++ body it restates;
  * non-vacuity: one-token mutations of the source that the bounds must reject;
  * lazy budgets: the operand codes of s2k_fp_op_batch_ex (ops.hip, fe29_lazy_form) each formula accepts, which the
    GPU test (test_gpu_fe29_formulas.py) runs at exactly their limit.
"""
import functools
import itertools
import os
import re

import pytest

import test_fe29_model as m
from test_fe29_model import B, L, M, M8, P_LIMBS, U32, W, add, cpp, mul, mul_add_mul, mul_int, mul_plus, mul_small_norm, \
    negate, normalize_weak, sqr, sqr_plus

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "secp256k1_voi_amd", "csrc")
NORM_IN = U32 - (1 << 18)         # fe29_normalize_weak: input limbs < 2^32 - 2^18


def join(*vs):
    return B([max(h) for h in zip(*(v.hi for v in vs))])


def le(a, b):
    return all(x <= y for x, y in zip(a.hi, b.hi))


CANON = B([M] * 8 + [M8])                 # fe29_from_words, fe29_normalize, fe29_inv_gcd
PROD = m.mulsum([(B.units(1), B.units(7.8))])  # what a product leaves at its full budget (limb 2 a little above 2^29)
NW = normalize_weak(B.units(7))           # what fe29_normalize_weak leaves
COORD = join(CANON, PROD, NW)             # "1 unit" as the formulas' coordinates carry it
TWO_P = B([2 * p for p in P_LIMBS])       # fe29_cond_negate1's result bound
Y2 = join(TWO_P, B.units(2))              # "y <= 2 units"


# ---- the primitives test_fe29_model.py does not have ----------------------------------------------------------------------
@cpp("fe29_one")
def one():
    return B([1] + [0] * 8)


@cpp("fe29_zero")
def zero():
    return B([0] * 9)


@cpp("fe29_from_words")
def from_words():
    return CANON


@cpp("fe29_select")
def select(a, b):
    return join(a, b)


@cpp("fe29_cond_negate1")
def cond_negate1(a, neg=None):
    """(a ^ M) + (M & (2p + 1)): 2p - a limb by limb when neg (no wrap only for a <= 2p limb-wise); None: either"""
    if neg is False:
        return a
    assert all(x <= 2 * p for x, p in zip(a.hi, P_LIMBS)), "cond_negate1 operand above 2p"
    return TWO_P if neg else join(a, TWO_P)


@cpp("fe29_normalize")
def normalize(a):
    assert all(h < NORM_IN for h in a.hi), "normalize input limb >= 2^32 - 2^18"
    normalize_weak(a)
    return CANON


@cpp("fe29_is_zero")
def is_zero(a):
    normalize.body(a)


@cpp("fe29_eq")
def eq(a, b):
    normalize.body(add.body(a, negate.body(b, 1)))


@cpp("fe29_inv_gcd")
def inv_gcd(a):
    return normalize.body(a)


@cpp("fe29_mul_small_lane")
def mul_small_lane(a, k):
    return mul_small_norm.body(a, k)


# quad values (pt29q.h): one bound per lane; a lane-wise call is one call of the C++ body.  Lane 3 "computes along":
# a lane whose operation overflows holds garbage (None) - harmless as long as no lane that is read later takes it.
class Quad(list):
    pass


def lanes(f):
    @cpp(f.cpp_name)
    def g(*args):
        out = Quad()
        for i in range(4):
            la = [a[i] if isinstance(a, Quad) else a for a in args]
            try:
                out.append(None if any(x is None for x in la) else f.body(*la))
            except AssertionError:
                out.append(None)
        return out
    return g


def live(r):
    assert all(x is not None for x in r), "a lane that is read took an overflowed value"
    return r


def per_lane(fn):
    return Quad(fn(q) for q in range(4))


@cpp("fe29_pick")
def pick(c, a, b):
    if isinstance(c, Quad):
        return Quad((b[i] if c[i] else a[i]) if isinstance(a, Quad) else (b if c[i] else a) for i in range(4))
    return join(a, b)


@cpp("fe29_qperm")
def qperm(sel, a):
    return Quad(a[s] for s in sel)


q_add, q_negate, q_mul, q_mul_plus, q_mul_add_mul, q_mul_int, q_normalize_weak, q_mul_small_norm, q_mul_small_lane, \
    q_cond_negate1 = map(lanes, (add, negate, mul, mul_plus, mul_add_mul, mul_int, normalize_weak, mul_small_norm,
                                 mul_small_lane, cond_negate1))


# ---- xyzz29.h -------------------------------------------------------------------------------------------------------------
@cpp("xyzz29_from_affine")
def xyzz_from_affine(bx, by):
    return (bx, by, one(), one())


@cpp("xyzz29_add_affine")
def xyzz_add_affine(p, bx, by):
    x, y, zz, zzz = p
    nx = negate(x, 1)
    pp_ = mul_plus(bx, zz, nx)
    rn = mul_plus(negate(by, 2), zzz, y)
    pp = sqr(pp_)
    pppn = mul(pp, negate(pp_, 1))
    qn = mul(nx, pp)
    rx = sqr_plus(rn, add(add(pppn, qn), qn))
    t = add(qn, rx)
    ry = mul_add_mul(t, rn, pppn, y)
    rzz = mul(zz, pp)
    rzzz = mul(zzz, negate(pppn, 1))
    return (rx, ry, rzz, rzzz)


@cpp("xyzz29_to_jacobian")
def xyzz_to_jacobian(p):
    x, y, zz, zzz = p
    return (mul(x, zz), mul(y, zzz), zz)


@cpp("xyzz29_from_jacobian")
def xyzz_from_jacobian(p):
    x, y, z = p
    zz = sqr(z)
    return (x, y, zz, mul(zz, z))


@cpp("xyzz29_to_pt29")
def xyzz_to_pt29(p):
    x, y, zz, zzz = p
    return (mul(x, zzz), mul(y, zz), mul(zz, zzz))


XYZZ_INV = (COORD, Y2, COORD, COORD)      # x [1], y [<= 2], zz [1], zzz [1]


def within(v, box):
    return all(le(a, b) for a, b in zip(v, box))


# ---- msm.hip: the bucket pass's addend and the redo path ---------------------------------------------------------------
@cpp("msm_point_of")
def msm_point_of():
    x = from_words()
    y = cond_negate1(from_words())
    return x, y


@cpp("pt29_identity")
def pt_identity():
    return (zero(), one(), zero())


@cpp("msm_piece")
def msm_piece(x):
    """the stored piece x; the redo loop's body once, on the accumulator bound PT_INV"""
    is_zero(x[2])
    xyzz_to_pt29(x)
    pt_identity()
    qx, qy = msm_point_of()
    return m.pt_add_mixed(PT_INV, qx, normalize_weak(qy))


PT_INV = (COORD, COORD, COORD)            # a pt29: x, y, z [1]


# ---- pt29q.h --------------------------------------------------------------------------------------------------------------
ROT = (1, 2, 0, 3)


@cpp("pt29q_add")
def ptq_add(pc, qc):
    T = q_mul(pc, qc)
    a = q_add(pc, qperm(ROT, pc))
    b = q_add(qc, qperm(ROT, qc))
    e = q_negate(q_add(T, qperm(ROT, T)), 2)
    U = q_mul_plus(a, b, e)
    Ts = q_mul_small_lane(T, per_lane(lambda q: 3 if q == 0 else (1 if q == 1 else 21)))
    Us = q_mul_small_lane(U, per_lane(lambda q: 21 if q >= 2 else 1))
    t1 = qperm((1, 1, 1, 1), Ts)
    t2 = qperm((2, 2, 2, 2), Ts)
    V = q_add(t1, q_cond_negate1(t2, per_lane(lambda q: q != 1)))
    Wq = q_add(t1, t2)
    A = pick(per_lane(lambda q: q >= 2), Us, Wq)
    C = qperm((1, 0, 2, 3), Us)
    Dr = pick(per_lane(lambda q: q >= 2), Ts, q_negate(Us, 1))
    D = qperm((2, 0, 0, 3), Dr)
    R = q_mul_add_mul(A, V, C, D)
    return live(qperm((0, 2, 1, 1), R))


@cpp("pt29q_double")
def ptq_double(pc):
    P = q_mul(qperm((0, 1, 2, 1), pc), qperm((1, 1, 2, 2), pc))
    t0 = qperm((1, 1, 1, 1), P)
    zz = qperm((2, 2, 2, 2), P)
    z3 = q_mul_int(q_normalize_weak(q_mul_int(t0, 4)), 2)
    t2 = q_mul_small_norm(zz, 21)
    y3 = q_add(t0, t2)
    t0m = q_normalize_weak(q_add(t0, q_negate(q_mul_small_norm(zz, 63), 1)))
    A = pick(per_lane(lambda q: q == 3), pick(per_lane(lambda q: q == 0), z3, P), y3)
    Bq = pick(per_lane(lambda q: q == 3),
              pick(per_lane(lambda q: q == 2), pick(per_lane(lambda q: q == 0), t2, q_mul_int(t0m, 2)), qperm((3, 3, 3, 3), P)),
              t0m)
    R = q_mul(A, Bq)
    S = q_normalize_weak(q_add(R, qperm((0, 3, 2, 3), R)))
    return live(qperm((0, 1, 2, 2), pick(per_lane(lambda q: q == 1), R, S)))


QUAD_INV = Quad([COORD] * 4)              # every lane's coordinate [1] (lane 3: a copy of Z)


# ---- aff29.h and the wide joint-table kernels of keyed.hip -----------------------------------------------------------------
@cpp("aff_double")
def aff_double(x, y):
    inv = inv_gcd(add(y, y))
    lam = mul(mul_int(sqr(x), 3), inv)
    x3 = sqr_plus(lam, negate(add(x, x), 2))
    y = mul_plus(lam, add(x, negate(x3, 1)), negate(y, 1))
    return x3, y


@cpp("aff_add")
def aff_add(x1, y1, x2, y2):
    di = inv_gcd(add(x2, negate(x1, 1)))
    nya = negate(y1, 1)
    lam = mul(add(y2, nya), di)
    x3 = sqr_plus(lam, negate(add(x1, x2), 2))
    y3 = mul_plus(lam, add(x1, negate(x3, 1)), nya)
    return x3, y3


@cpp("k_ksw_odd")
def ksw_odd(x, y, ne=16, r=3):
    """B_i from a stored chunk entry by r doublings, 2 B_i, then the odd multiples by repeated addition of 2 B_i"""
    for _ in range(r):
        x, y = aff_double(x, y)
    outs = [(x, y)]
    dx, dy = aff_double(x, y)
    for _ in range(1, ne):
        x, y = aff_add(x, y, dx, dy)
        outs.append((x, y))
    return outs


@cpp("k_ksw_lead")
def ksw_lead(x, y, shift=4):
    for _ in range(shift):
        x, y = aff_double(x, y)
    return x, y


def _joint_pair(ya, yb, xa, bxb, di):
    """one (a, b) pair of k_ks_joint / k_ksw_joint, both signs joined"""
    nxs = negate(add(xa, bxb), 2)
    nya = negate(ya, 1)
    dy = join(negate(add(yb, ya), 2), add(yb, nya))
    lam = mul(dy, di)
    x3 = sqr_plus(lam, nxs)
    y3 = mul_plus(lam, add(xa, negate(x3, 1)), nya)
    return x3, y3


@cpp("k_ks_joint")
def ks_joint(e):
    """e: the bound of a stored 32-chunk entry's x, y and beta x; the loops' bodies once each"""
    pre = one()
    d = add(e, negate(e, 1))
    pre = mul(pre, d)
    inv = inv_gcd(pre)
    d = add(e, negate(e, 1))
    prev = join(one(), PROD)
    di = mul(inv, prev)
    inv = mul(inv, d)
    return _joint_pair(e, e, e, e, di)


@cpp("k_ksw_joint")
def ksw_joint(e):
    """e: the bound of an odd-multiple entry's x and y (k_ksw_odd's outputs)"""
    beta = from_words()
    pre = one()
    d = add(mul(e, beta), negate(e, 1))
    pre = mul(pre, d)
    inv = inv_gcd(pre)
    bxb = mul(e, beta)
    d = add(bxb, negate(e, 1))
    prev = join(one(), PROD)
    di = mul(inv, prev)
    inv = mul(inv, d)
    return _joint_pair(e, e, e, bxb, di)


# ---- the per-key chunk tables of keyed.hip ------------------------------------------------------------------------------
SEVEN = B([7] + [0] * 8)                  # rhs.n[0] += 7


@cpp("fe29_sqrt")
def sqrt(a):
    """a^((p+1)/4): the fe29_pow_x223 chain takes products with a (a of 1 unit), then fe29_eq(fe29_sqr(t), a)"""
    t = mul.body(PROD, a)
    eq.body(sqr.body(t), a)
    return PROD


@cpp("k_key_chain")
def key_chain(nd=1):
    """both key forms (x-only lifted to the even y, 64-byte X || Y checked on the curve), nd doublings of the chain,
    then the lead pair L +- phi(L) by one co-Z addition; returns the last chunk point and the two lead points"""
    qx = from_words()
    rhs = add.body(mul(sqr(qx), qx), SEVEN)
    qy = sqrt(rhs)
    qx, qy = join(qx, from_words()), join(qy, from_words())
    qy = normalize(qy)
    qy = select(qy, normalize_weak(negate(qy, 1)))
    xo, yo = qx, qy
    qx = from_words()
    qy = from_words()
    rhs = add.body(mul(sqr(qx), qx), SEVEN)
    eq(sqr(qy), rhs)
    qx, qy = join(qx, from_words(), xo), join(qy, from_words(), yo)
    cur = (qx, qy, one())
    for _ in range(nd):
        cur = m.jpt_double(*cur)
    bx = mul(cur[0], from_words())
    h = normalize_weak(add(bx, negate(cur[0], 1)))
    z3 = mul(cur[2], h)
    a = sqr(h)
    b = mul(cur[0], a)
    c = mul(bx, a)
    bc = add(b, c)
    yn = normalize_weak(cur[1])
    xs = normalize_weak(negate(bc, 2))
    ys = mul(negate(yn, 1), normalize_weak(add(c, negate(b, 1))))
    xd = normalize_weak(add(sqr(mul_int(yn, 2)), negate(bc, 2)))
    yd = mul(negate(yn, 1), normalize_weak(add(bc, negate(mul_int(xd, 2), 2))))
    return cur, (xs, ys, z3), (xd, yd, z3)


@cpp("k_key_cofactors")
def key_cofactors(z, lead, st):
    """one trip of every loop of both geometries (CHUNKS == 8: prefix products in registers; 32: through the scratch).
    z: a chunk's stored Z, lead: the lead points' x, y, x, y, st: the running prefix / suffix products of both forms"""
    lx, ly, dx, dy = lead
    pre8, suf8, pre32, suf32 = st
    pre8 = mul(pre8, z)
    s1 = one()
    co = join(pre8, mul(pre8, suf8), suf8)
    s2 = sqr(co)
    s3 = mul(s2, co)
    outs = [mul(lx, s2), mul(ly, s3), zero(), mul(dx, s2), mul(dy, s3), zero(), co]
    suf8 = join(z, mul(suf8, z), s1)
    pre32 = mul(pre32, z)
    outs.append(mul(pre32, lead[0]))
    s2 = sqr(pre32)
    s3 = mul(s2, pre32)
    outs += [mul(lx, s2), mul(ly, s3), zero(), mul(dx, s2), mul(dy, s3), zero()]
    outs.append(join(mul(pre32, suf32), suf32))
    suf32 = mul(suf32, z)
    return (pre8, suf8, pre32, suf32), outs


def cofactors_run(chunks=8, mutation=None):
    """k_key_cofactors over all chunks of a key: the source (or the mutated source) once per chunk"""
    st = (COORD,) * 4
    for _ in range(chunks):
        st, outs = m.mutated(key_cofactors, mutation, COORD, (NW, PROD, NW, PROD), st) if mutation else \
            key_cofactors(COORD, (NW, PROD, NW, PROD), st)
        assert all(le(o, COORD) for o in outs), "a stored cofactor product is above 1 unit"
    return st


@cpp("k_key_odd")
def key_odd(ex, ey, ezb):
    """entry 0 of a chunk (x, y as k_key_chain stores them, zb its Z) -> the eight odd multiples; loop body once"""
    a0 = (ex, ey, one())
    zb = ezb
    d = m.jpt_double(*a0)
    c2 = sqr(d[2])
    c3 = mul(c2, d[2])
    cur = (mul(a0[0], c2), mul(a0[1], c3), one())
    x, y, z, h = m.jpt_add_affine(*cur, d[0], d[1])
    return x, y, h, mul(mul(z, d[2]), zb)


@cpp("k_key_scale")
def key_scale(ex, ey, eh, rr):
    beta = from_words()
    r2 = sqr(rr)
    r3 = mul(r2, rr)
    x = mul(ex, r2)
    y = mul(ey, r3)
    rr = mul(rr, eh)
    return x, y, mul(x, beta)


@cpp("fe29_group_shl")
def group_shl(a):
    return join(a, one.body())


@cpp("k_key_scale_wide")
def key_scale_wide(x, y, h, co):
    s = group_shl(h)
    s = mul(s, group_shl(s))
    s = mul(s, group_shl(s))
    s = mul(s, group_shl(s))
    rr = mul(co, s)
    r2 = sqr(rr)
    r3 = mul(r2, rr)
    xs = mul(x, r2)
    ys = mul(y, r3)
    return xs, ys, mul(xs, from_words())


# ==== bounds and closure =====================================================================================================
def test_xyzz_bucket_pass_invariant_closed():
    # the addend: canonical x, y through fe29_cond_negate1 (msm_point_of) - y <= 2p limb by limb, i.e. <= 2 units
    bx, by = msm_point_of()
    assert le(bx, COORD) and le(by, Y2)
    acc = xyzz_from_affine(bx, by)
    assert within(acc, XYZZ_INV)
    acc = XYZZ_INV
    for _ in range(3):
        acc = xyzz_add_affine(acc, bx, by)
        assert within(acc, XYZZ_INV), [a.hi for a in acc]
    # the keyed ladder's addend: a stored product through cond_negate1, and its round border (verify_fast.h)
    acc = xyzz_add_affine(XYZZ_INV, PROD, cond_negate1(PROD))
    j = xyzz_to_jacobian(acc)
    for _ in range(4):
        j = m.jpt_double(*j)
        assert le(j[0], COORD) and le(j[1], Y2) and le(j[2], COORD)
    acc = xyzz_from_jacobian(j)
    assert within(acc, XYZZ_INV)
    # the pieces as k_msm_stitch / k_msm_fold see them: pt29 coordinates of 1 unit
    assert within(xyzz_to_pt29(XYZZ_INV), PT_INV)


def test_xyzz_budgets():
    # the largest inputs the addition takes: x, zz, zzz at 1 unit (negate(x, 1)), y up to what the products allow,
    # the addend's y up to 3 units' bias (negate(by, 2))
    y_max = B.units(3.8)
    xyzz_add_affine((COORD, y_max, COORD, COORD), COORD, B(3 * p for p in P_LIMBS))
    with pytest.raises(AssertionError):
        xyzz_add_affine((COORD, B.units(6), COORD, COORD), COORD, TWO_P)


def test_redo_and_stitch_paths():
    # msm_piece: a stored piece of the XYZZ invariant, the complete formulas on the accumulator and the addend
    r = msm_piece(XYZZ_INV)
    assert within(r, PT_INV)
    # k_msm_stitch / k_msm_stitch_big / k_msm_fold: pt29_add of pieces as xyzz29_to_pt29 leaves them, and of sums
    piece = xyzz_to_pt29(XYZZ_INV)
    assert within(m.pt_add(piece, piece), PT_INV) and within(m.pt_add(PT_INV, piece), PT_INV)
    assert within(m.pt_add(PT_INV, PT_INV), PT_INV) and within(m.pt_double(PT_INV), PT_INV)


def test_pt29q_invariant_closed():
    # every lane's coordinate stays [1] under additions and doublings in any order (the bucket reduction, tree, Horner tail)
    for f in (lambda a: ptq_add(a, QUAD_INV), lambda a: ptq_double(a), lambda a: ptq_add(QUAD_INV, a)):
        r = f(QUAD_INV)
        assert all(le(r[i], COORD) for i in range(4)), [x.hi for x in r]
    # pt29q_from of a point from words / of a pt29: lanes as the invariant
    assert all(le(x, COORD) for x in ptq_add(Quad([CANON] * 4), Quad([NW] * 4)))


def test_aff_formulas_invariant_closed():
    # "operands and results with 1 unit": the inversions take 2y [2] and x2 - x1 [3], below normalize's input bound
    for x, y in ((CANON, CANON), (PROD, PROD), (COORD, COORD)):
        x3, y3 = aff_double(x, y)
        assert le(x3, COORD) and le(y3, COORD)
        x3, y3 = aff_add(x, y, x, y)
        assert le(x3, COORD) and le(y3, COORD)
    # k_ksw_odd / k_ksw_lead feed their results back in: the stored chunk entries are products
    outs = ksw_odd(PROD, PROD)
    assert all(le(x, COORD) and le(y, COORD) for x, y in outs)
    x, y = ksw_lead(PROD, PROD)
    assert le(x, COORD) and le(y, COORD)
    # and the joint tables built from them
    x3, y3 = ksw_joint(COORD)
    assert le(x3, COORD) and le(y3, COORD)
    x3, y3 = ks_joint(COORD)
    assert le(x3, COORD) and le(y3, COORD)


def test_aff_budgets():
    # aff_double: x at most 1.5 p limb-wise (negate(x + x, 2)), y at most 2 p (negate(y, 1))
    xb, yb = B([3 * p // 2 for p in P_LIMBS]), TWO_P
    aff_double(xb, yb)
    with pytest.raises(AssertionError):
        aff_double(B.units(2), COORD)
    with pytest.raises(AssertionError):
        aff_double(COORD, B.units(3))
    # aff_add: x1 <= 2p (negate(x1, 1)), x1 + x2 <= 3p, y1 <= 2p, y2 + 2 units within the product budget
    aff_add(COORD, TWO_P, COORD, B.units(3))
    with pytest.raises(AssertionError):
        aff_add(COORD, B.units(3), COORD, COORD)


def test_key_chain_and_cofactors():
    # k_key_chain: the key's point (canonical x, y; the x-only lift's even y weakly normalised), 116 / 128 doublings in
    # chunks of 4; every stored chunk point stays a jpt29 (x [1], y [<= 2], z [1]); the lead pair is stored at 1 unit
    cur, lead_s, lead_d = key_chain(1)
    for _ in range(8):
        assert le(cur[0], COORD) and le(cur[1], Y2) and le(cur[2], COORD)
        cur = m.jpt_double(*cur)
    assert all(le(v, COORD) for v in lead_s + lead_d)
    # k_key_cofactors: prefix and suffix products over the chunks of a key stay products
    st = cofactors_run(8)
    assert all(le(v, COORD) for v in st)
    cofactors_run(32)


def test_key_cofactors_mutation():
    # fe29_mul(pre[c - 1], z[c]) -> fe29_add: the prefix grows by a unit per chunk and its square overflows
    with pytest.raises(AssertionError):
        cofactors_run(8, ("fe29_mul", 0, (add, lambda a: a)))


def test_key_table_kernels():
    # k_key_chain stores x, y, z of jpt29 points (x [1], y [<= 2], z [1]); the odd multiples from them
    x, y, h, zc = key_odd(COORD, Y2, COORD)
    assert le(x, COORD) and le(y, COORD) and le(h, COORD) and le(zc, COORD)
    # k_key_scale / k_key_scale_wide rescale entries (x [1], y [1], H [1]) by cofactor products
    for f in (key_scale, key_scale_wide):
        xs, ys, bx = f(COORD, COORD, COORD, COORD)
        assert le(xs, COORD) and le(ys, COORD) and le(bx, COORD)


# ==== call sites of fe29_eq / fe29_is_zero / fe29_normalize / fe29_inv_gcd ==================================================
RHS = add.body(PROD, B([7] + [0] * 8))                  # fe29_mul(fe29_sqr(x), x) with 7 added to limb 0
SEL_NEG = join(CANON, NW)                                 # select(odd, y, normalize_weak(negate(y, 1)))
SEL_RAW = join(CANON, negate.body(CANON, 1))              # select(odd, y, negate(y, 1))
FER1 = B.units(1)                                         # fe29r.h: fer_norm / fer_mul results, one unit (tests/fer_model.py)

# (file, text of the call as the source has it, how often, check)
CALL_SITES = [
    ("verify_fast.h", "fe29_eq(fe29_sqr(qy), rhs)", 1, lambda: eq(PROD, RHS)),
    ("verify_fast.h", "fe29_is_zero(acc.z)", 3, lambda: is_zero(COORD)),
    ("verify_fast.h", "qy = fe29_normalize(qy)", 2, lambda: normalize(PROD)),        # fe29_sqrt's root, or words
    ("verify_fast.h", "fe29_is_zero(q.z)", 1, lambda: is_zero(COORD)),
    ("verify_fast.h", "fe29_is_zero(acc.x)", 1, lambda: is_zero(COORD)),
    ("verify_fast.h", "fe29_eq(acc.x, fe29_mul(fe29_from_words(rw), zz))", 1, lambda: eq(COORD, PROD)),
    ("verify_fast.h", "fe29_eq(acc.x, fe29_mul(fe29_from_words(r2), zz))", 1, lambda: eq(COORD, PROD)),
    ("worklist.hip", "fe29_eq(fe29_sqr(qy), rhs)", 1, lambda: eq(PROD, RHS)),
    ("worklist.hip", "fe29_is_zero(acc.z)", 1, lambda: is_zero(COORD)),
    ("worklist.hip", "fe29_eq(acc.x, fe29_mul(fe29_from_words(r.v), acc.z))", 1, lambda: eq(COORD, PROD)),
    ("worklist.hip", "fe29_eq(acc.x, fe29_mul(fe29_from_words(r2), acc.z))", 1, lambda: eq(COORD, PROD)),
    ("worklist.hip", "y = fe29_normalize(y)", 1, lambda: normalize(PROD)),
    ("lane_kernels.hip", "fe29_inv_gcd(acc)", 1, lambda: inv_gcd(PROD)),
    ("lane_kernels.hip", "fe29_normalize(fe29_mul(fe29_mul(fq_load(fin, stride, i, 1), zi2), zi))", 1, lambda: normalize(PROD)),
    ("lane_kernels.hip", "fe29_normalize(x)", 1, lambda: normalize(PROD)),
    ("lane_kernels.hip", "fe29_eq(x, fe29_from_words(rw))", 1, lambda: eq(PROD, CANON)),
    ("worklist.hip", "fe29_is_zero(p.z)", 1, lambda: is_zero(COORD)),
    ("worklist.hip", "fe29_inv_gcd(fe29_normalize_weak(p.z))", 1, lambda: inv_gcd(NW)),
    ("worklist.hip", "fe29_normalize(fe29_mul(p.x, zi))", 1, lambda: normalize(PROD)),
    ("worklist.hip", "fe29_normalize(fe29_mul(p.y, zi))", 1, lambda: normalize(PROD)),
    ("small_call.hip", "fe29_eq(fe29_sqr(qy), rhs)", 1, lambda: eq(PROD, RHS)),                 # k_verify_quad
    ("small_call.hip", "qy = fe29_normalize(qy)", 1, lambda: normalize(PROD)),                   # k_recover_quad: fe29_sqrt's root
    ("small_call.hip", "fe29_is_zero(fer_to_fe29(fer_norm(a, k)))", 1, lambda: is_zero(FER1)),
    ("small_call.hip", "fe29_normalize(fer_to_fe29(fer_norm(a, k)))", 1, lambda: normalize(FER1)),
    ("small_call.hip", "fe29_is_zero(R.z)", 3, lambda: is_zero(COORD)),
    ("small_call.hip", "fe29_eq(R.x, fe29_mul(fe29_from_words(rw), R.z))", 1, lambda: eq(COORD, PROD)),
    ("small_call.hip", "fe29_eq(R.x, fe29_mul(fe29_from_words(r2), R.z))", 1, lambda: eq(COORD, PROD)),
    ("small_call.hip", "y = fe29_normalize(y)", 1, lambda: normalize(PROD)),                     # k_schnorr_quad
    ("small_call.hip", "fe29_eq(R.x, fe29_mul(xR, R.z))", 1, lambda: eq(COORD, PROD)),
    ("small_call.hip", "fe29_eq(R.y, fe29_mul(yR, R.z))", 1, lambda: eq(COORD, PROD)),
    ("small_call.hip", "fe29_normalize(fer_to_fe29(fer_mul(acc.x, zi, k)))", 1, lambda: normalize(FER1)),
    ("small_call.hip", "fe29_normalize(fer_to_fe29(fer_mul(fer_norm(acc.y, k), zi, k)))", 1, lambda: normalize(FER1)),
    ("keyed.hip", "qy = fe29_normalize(qy)", 1, lambda: normalize(PROD)),
    ("keyed.hip", "fe29_eq(fe29_sqr(qy), rhs)", 1, lambda: eq(PROD, RHS)),
    ("keyed.hip", "fe29_inv_gcd(pre)", 2, lambda: inv_gcd(PROD)),
    ("aff29.h", "fe29_inv_gcd(fe29_add(y, y))", 1, lambda: inv_gcd(add.body(TWO_P, TWO_P))),
    ("aff29.h", "fe29_inv_gcd(fe29_add(x2, fe29_negate(x1, 1)))", 1,
     lambda: inv_gcd(add.body(B([3 * p // 2 for p in P_LIMBS]), negate.body(TWO_P, 1)))),
    ("msm_terms.h", "fe29_normalize(fe29_mul(fe29_from_words(x), fe29_from_words(FE_BETA)))", 1, lambda: normalize(PROD)),
    ("msm_terms.h", "fe29_eq(fe29_sqr(y), rhs)", 1, lambda: eq(PROD, RHS)),
    ("msm.hip", "fe29_is_zero(x.zz)", 1, lambda: is_zero(COORD)),
    ("msm.hip", "fe29_is_zero(acc.z)", 2, lambda: is_zero(COORD)),
    ("msm.hip", "fe29_inv_gcd(fe29_normalize_weak(acc.z))", 2, lambda: inv_gcd(NW)),
    ("msm.hip", "fe29_normalize(fe29_mul(acc.x, zi))", 2, lambda: normalize(PROD)),
    ("msm.hip", "fe29_normalize(fe29_mul(acc.y, zi))", 2, lambda: normalize(PROD)),
    ("rlc.hip", "y = fe29_normalize(y)", 1, lambda: normalize(PROD)),
    ("rlc.hip", "fe29_normalize(fe29_select((y.n[0] & 1u) != 0, y, fe29_negate(y, 1)))", 1, lambda: normalize(SEL_RAW)),
]
ROOTS = re.compile(r"\bfe29_(?:eq|is_zero|normalize|inv_gcd)\s*\(")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        s = f.read()
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", "", s)


def test_call_site_table_is_complete():
    # (engine.hip's kernels moved to verify_fast.h, lane_kernels.hip, fallback.hip and worklist.hip: 10 + 4 + 0 + 9 call sites, the
    # 23 engine.hip had; engine.hip and the ladder units stay in the list so that a call that turns up there needs a row)
    for f in ("engine.hip", "verify_fast.h", "lane_kernels.hip", "fallback.hip", "worklist.hip", "ladder_ecdsa.hip", "ladder_schnorr.hip",
              "small_call.hip", "gtable.hip", "keyed.hip", "msm.hip", "msm_terms.h", "msm_internal.h", "rlc.hip", "aff29.h"):
        rows = [r for r in CALL_SITES if r[0] == f]
        s = source(f)
        assert len(ROOTS.findall(s)) == sum(r[2] for r in rows), f"{f}: a call of fe29_eq / is_zero / normalize / inv_gcd has no row"
        for _, text, count, _check in rows:
            assert s.count(text) == count, (f, text)


@pytest.mark.parametrize("row", CALL_SITES, ids=[f"{r[0]}:{r[1]}" for r in CALL_SITES])
def test_call_site_operand_bounds(row):
    row[3]()


def test_normalize_contract_rejects():
    with pytest.raises(AssertionError):
        normalize(B.units(8))
    with pytest.raises(AssertionError):
        eq(PROD, B.units(2))


# ==== drift guard ============================================================================================================
TRACKED = re.compile(r"\b(fe29_\w+|pt29\w*|xyzz29_\w+|jpt29_\w+|aff_\w+|msm_point_of)\b")


def body_of(fname, func):
    s = source(fname)
    for mt in re.finditer(r"\b%s\s*\(" % re.escape(func), s):
        i, depth = mt.end() - 1, 0
        while True:                                   # the parameter list
            depth += {"(": 1, ")": -1}.get(s[i], 0)
            i += 1
            if depth == 0:
                break
        rest = s[i:].lstrip()
        if not rest.startswith("{"):
            continue                                  # a call, not the definition
        j = s.index("{", i)
        depth, k = 0, j
        while True:
            depth += {"{": 1, "}": -1}.get(s[k], 0)
            k += 1
            if depth == 0:
                return s[j + 1:k - 1]
    raise AssertionError(f"no definition of {func} in {fname}")


def calls_in(body):
    """the tracked calls of a C++ body in evaluation order: a call after its arguments, arguments left to right"""
    out, stack, i = [], [], 0
    while i < len(body):
        mt = TRACKED.match(body, i) if (i == 0 or not (body[i - 1].isalnum() or body[i - 1] == "_")) else None
        if mt:
            j = mt.end()
            if body.startswith("<", j):               # template arguments
                d = 0
                while True:
                    d += {"<": 1, ">": -1}.get(body[j], 0)
                    j += 1
                    if d == 0:
                        break
            while j < len(body) and body[j].isspace():
                j += 1
            if j < len(body) and body[j] == "(":
                stack.append(mt.group(1))
                i = j + 1
                continue
            i = mt.end()
            continue
        c = body[i]
        if c == "(":
            stack.append(None)
        elif c == ")":
            name = stack.pop()
            if name:
                out.append(name)
        i += 1
    return out


Q1 = Quad([COORD] * 4)
# model function, its inputs, where the C++ body is
GUARDED = [
    (m.jpt_double, (COORD, Y2, COORD), "jacobian29.h", "jpt29_double"),
    (m.jpt_add_affine, (COORD, Y2, COORD, COORD, Y2), "jacobian29.h", "jpt29_add_affine"),
    (m.pt_add_tail, (PROD,) * 6, "pt29.h", "pt29_add_tail"),
    (m.pt_add, (PT_INV, PT_INV), "pt29.h", "pt29_add"),
    (m.pt_add_mixed, (PT_INV, CANON, NW), "pt29.h", "pt29_add_mixed"),
    (m.pt_double, (PT_INV,), "pt29.h", "pt29_double"),
    (xyzz_from_affine, (COORD, Y2), "xyzz29.h", "xyzz29_from_affine"),
    (xyzz_add_affine, (XYZZ_INV, COORD, Y2), "xyzz29.h", "xyzz29_add_affine"),
    (xyzz_to_jacobian, (XYZZ_INV,), "xyzz29.h", "xyzz29_to_jacobian"),
    (xyzz_from_jacobian, ((COORD, Y2, COORD),), "xyzz29.h", "xyzz29_from_jacobian"),
    (xyzz_to_pt29, (XYZZ_INV,), "xyzz29.h", "xyzz29_to_pt29"),
    (ptq_add, (Q1, Q1), "pt29q.h", "pt29q_add"),
    (ptq_double, (Q1,), "pt29q.h", "pt29q_double"),
    (mul_small_lane, (PROD, 21), "pt29q.h", "fe29_mul_small_lane"),
    (msm_point_of, (), "msm.hip", "msm_point_of"),
    (msm_piece, (XYZZ_INV,), "msm.hip", "msm_piece"),
    (aff_double, (COORD, COORD), "aff29.h", "aff_double"),
    (aff_add, (COORD, COORD, COORD, COORD), "aff29.h", "aff_add"),
    (lambda x, y: ksw_odd.body(x, y, 2, 1), (COORD, COORD), "keyed.hip", "k_ksw_odd"),
    (lambda x, y: ksw_lead.body(x, y, 1), (COORD, COORD), "keyed.hip", "k_ksw_lead"),
    (ks_joint, (COORD,), "keyed.hip", "k_ks_joint"),
    (ksw_joint, (COORD,), "keyed.hip", "k_ksw_joint"),
    (key_odd, (COORD, Y2, COORD), "keyed.hip", "k_key_odd"),
    (key_scale, (COORD, COORD, COORD, COORD), "keyed.hip", "k_key_scale"),
    (key_scale_wide, (COORD, COORD, COORD, COORD), "keyed.hip", "k_key_scale_wide"),
    (group_shl, (COORD,), "keyed.hip", "fe29_group_shl"),
    (key_chain, (), "keyed.hip", "k_key_chain"),
    (key_cofactors, (COORD, (NW, PROD, NW, PROD), (COORD,) * 4), "keyed.hip", "k_key_cofactors"),
]


@pytest.mark.parametrize("g", GUARDED, ids=[g[3] for g in GUARDED])
def test_drift_guard(g):
    fn, args, fname, func = g
    assert m.record(fn, *args) == calls_in(body_of(fname, func)), f"{func} ({fname}) no longer matches its model"


def test_drift_guard_sees_an_edit():
    body = body_of("xyzz29.h", "xyzz29_add_affine")
    edited = body.replace("fe29_mul(nx, pp)", "fe29_sqr(nx)", 1)
    assert edited != body and calls_in(edited) != m.record(xyzz_add_affine, XYZZ_INV, COORD, Y2)
    assert calls_in("a = fe29_qperm<S2K_QP(1, 2, 0, 3)>(fe29_add(x, y)); b = fe29_group_shl<1>(s, j < 7);") == \
        ["fe29_add", "fe29_qperm", "fe29_group_shl"]


# ==== non-vacuity: one-token mutations of the source that the model rejects ====================================================
def _lower(args):
    return (args[0], args[1] - 1)


def _swap(other):
    """the call replaced by a call of `other` on the same arguments (one token: the function's name)"""
    return (other, lambda args: args)


XYZZ_BOX, JPT_BOX = (COORD, Y2, COORD, COORD), (COORD, Y2, COORD)
MUTATIONS = [
    # (name, model, inputs, mutation (call, occurrence, change[, deep]), boxes the outputs must stay in or None)
    ("xyzz29_add_affine: fe29_negate(p.x, 1) -> 0", xyzz_add_affine, (XYZZ_INV, COORD, TWO_P), ("fe29_negate", 0, _lower), XYZZ_BOX),
    ("xyzz29_add_affine: fe29_negate(by, 2) -> 0 (the bucket-pass addend, 2p - y)", xyzz_add_affine, (XYZZ_INV, COORD, TWO_P),
     ("fe29_negate", 1, lambda a: (a[0], 0)), XYZZ_BOX),
    ("xyzz29_add_affine: fe29_negate(pppn, 1) -> 0", xyzz_add_affine, (XYZZ_INV, COORD, TWO_P), ("fe29_negate", 3, _lower), XYZZ_BOX),
    ("xyzz29_to_jacobian: fe29_mul(p.x, p.zz) -> fe29_add", xyzz_to_jacobian, (XYZZ_INV,), ("fe29_mul", 0, _swap(add)), JPT_BOX),
    ("xyzz29_from_jacobian: fe29_mul(r.zz, p.z) -> fe29_add", xyzz_from_jacobian, (JPT_BOX,), ("fe29_mul", 0, _swap(add)),
     XYZZ_BOX),
    ("xyzz29_to_pt29: fe29_mul(p.x, p.zzz) -> fe29_add", xyzz_to_pt29, (XYZZ_INV,), ("fe29_mul", 0, _swap(add)), PT_INV),
    ("pt29q_add: fe29_negate(fe29_add(T, ..), 2) -> 1", ptq_add, (Q1, Q1), ("fe29_negate", 0, _lower), None),
    ("pt29q_add: fe29_negate(Us, 1) -> 0", ptq_add, (Q1, Q1), ("fe29_negate", 1, _lower), None),
    ("pt29q_double: fe29_negate(fe29_mul_small_norm(zz, 63), 1) -> 0", ptq_double, (Q1,), ("fe29_negate", 0, _lower), None),
    ("pt29q_double: fe29_normalize_weak(fe29_add(R, ..)) -> fe29_add(R, ..) (Y3 leaves with 2 units)", ptq_double, (Q1,),
     ("fe29_normalize_weak", 2, None), (COORD,) * 4),
    ("msm_point_of: fe29_cond_negate1 -> fe29_negate (a non-negative entry: w = 0)", msm_point_of, (),
     ("fe29_cond_negate1", 0, (negate, lambda a: (a[0], 0))), None),
    ("msm_piece: the same edit of msm_point_of, on the redo path", msm_piece, (XYZZ_INV,),
     ("fe29_cond_negate1", 0, (negate, lambda a: (a[0], 0)), True), None),
    ("aff_double: fe29_negate(fe29_add(x, x), 2) -> 1", aff_double, (COORD, COORD), ("fe29_negate", 0, _lower), None),
    ("aff_add: fe29_negate(fe29_add(x1, x2), 2) -> 1", aff_add, (COORD, COORD, COORD, COORD), ("fe29_negate", 2, _lower), None),
    ("aff_add: fe29_negate(y1, 1) -> 0", aff_add, (COORD, COORD, COORD, COORD), ("fe29_negate", 1, _lower), None),
    ("k_ksw_odd: aff_add's fe29_negate(y1, 1) -> 0", lambda x, y: ksw_odd.body(x, y, 2, 1), (PROD, PROD),
     ("fe29_negate", 7, _lower, True), None),     # (three negates in each of the two aff_double first)
    ("k_ksw_lead: aff_double's fe29_negate(fe29_add(x, x), 2) -> 1", lambda x, y: ksw_lead.body(x, y, 1), (PROD, PROD),
     ("fe29_negate", 0, _lower, True), None),
    ("k_ks_joint: fe29_negate(fe29_add(xa, bxb), 2) -> 1", ks_joint, (COORD,), ("fe29_negate", 2, _lower), None),
    ("k_ksw_joint: fe29_negate(xa, 1) -> 0", ksw_joint, (COORD,), ("fe29_negate", 0, _lower), None),
    ("k_key_chain: fe29_negate(bc, 2) -> 1", key_chain, (), ("fe29_negate", 2, _lower), None),
    ("k_key_odd: jpt29_double's fe29_negate(s, 1) -> 0", key_odd, (COORD, Y2, COORD), ("fe29_negate", 0, _lower, True), None),
    ("k_key_scale: fe29_mul(cx, r2) -> fe29_add", key_scale, (COORD,) * 4, ("fe29_mul", 1, _swap(add)), (COORD,) * 3),
    ("k_key_scale_wide: fe29_mul(x, r2) -> fe29_add", key_scale_wide, (COORD,) * 4, ("fe29_mul", 5, _swap(add)), (COORD,) * 3),
    ("pt29_double: drop fe29_normalize_weak of t0m", m.pt_double, (PT_INV,), ("fe29_normalize_weak", 1, None), None),
    ("pt29_add_mixed: fe29_negate(t0 + t1, 2) -> 1", m.pt_add_mixed, (PT_INV, CANON, NW), ("fe29_negate", 0, _lower), None),
    ("pt29_add: fe29_negate(t1 + t2, 2) -> 1", m.pt_add, (PT_INV, PT_INV), ("fe29_negate", 1, _lower), None),
    ("pt29_add_tail: fe29_negate(t2, 1) -> 0", m.pt_add_tail, (PROD,) * 6, ("fe29_negate", 0, _lower), None),
    ("jpt29_double: fe29_negate(s, 1) -> 0", m.jpt_double, (COORD, Y2, COORD), ("fe29_negate", 0, _lower), None),
    ("jpt29_add_affine: fe29_negate(p.x, 1) -> 0", m.jpt_add_affine, (COORD, Y2, COORD, COORD, TWO_P), ("fe29_negate", 0, _lower),
     None),
]


def _outputs_ok(r, boxes):
    if boxes is None:
        return True
    return all(le(x, b) for x, b in zip(r, boxes))


@pytest.mark.parametrize("mu", MUTATIONS, ids=[mu[0] for mu in MUTATIONS])
def test_mutation_is_rejected(mu):
    name, fn, args, mutation, boxes = mu
    assert _outputs_ok(fn(*args), boxes)             # the unmutated model passes on the same inputs
    try:
        r = m.mutated(fn, mutation, *args)
    except AssertionError:
        return
    assert not _outputs_ok(r, boxes), f"the model accepts the mutation {name}"


def test_mutation_the_bounds_accept():
    # fe29_negate(by, 2) -> 1 in the XYZZ addition is harmless: every addend the callers pass (cond_negate1's 2p - y,
    # a weakly normalised or canonical y) is at most 2p limb by limb
    for by in (TWO_P, NW, CANON):
        assert _outputs_ok(m.mutated(xyzz_add_affine, ("fe29_negate", 1, _lower), XYZZ_INV, COORD, by), XYZZ_BOX)


def test_msm_piece_addend_slack():
    # the redo path's fe29_normalize_weak(qy) is not needed for the bounds: the complete mixed addition takes an addend
    # y of 2 units (cond_negate1's result) as long as x has 1 - (qx + qy) (px + py) = 3 * 2 units
    assert within(m.mutated(msm_piece, ("fe29_normalize_weak", 0, None), XYZZ_INV), PT_INV)


def test_mutated_addend_is_rejected():
    # the bucket pass's addend with one unit more than cond_negate1 leaves (y [3] instead of [2])
    with pytest.raises(AssertionError):
        xyzz_add_affine(XYZZ_INV, COORD, B.units(3))
    with pytest.raises(AssertionError):
        cond_negate1(B.units(2.01))


# ==== lazy-code budgets of the s2k_fp_op_batch_ex forms (ops.hip) ==========================================================
def lazy_bound(code):
    """limb bounds of fe29_lazy_form(canonical, code): + k p limb by limb, bit 2 borrows 2^29 into limbs 0..7"""
    k, spread = code & 3, (code >> 2) & 1
    return B([M + spread * (1 << W) + k * P_LIMBS[i] for i in range(8)] + [M8 + k * P_LIMBS[8]])


def _aff_dbl(c):
    aff_double(lazy_bound(c[0]), lazy_bound(c[1]))


def _aff_add(c):
    aff_add(lazy_bound(c[0]), lazy_bound(c[1]), lazy_bound(c[2]), lazy_bound(c[3]))


def _pt29_add_mixed(c):
    # PT29_ADD_MIXED: P = (a c : b c : c) with c weakly normalised, Q = (d, e) taken as they are
    m.pt_add_mixed(PT_INV, lazy_bound(c[0]), lazy_bound(c[1]))


def _xyzz_lift(c):
    # XYZZ_ADD / XYZZ_ROUND: P = (a c^2, b c^3, c^2, c^3); Q = (d, e) weakly normalised
    a, b, cc = map(lazy_bound, c)
    c2 = sqr.body(cc)
    c3 = mul.body(c2, cc)
    return (mul.body(a, c2), mul.body(b, c3), c2, c3)


def _xyzz_add(c):
    xyzz_to_pt29(xyzz_add_affine(_xyzz_lift(c), NW, NW))


def _xyzz_round(c):
    # the keyed ladder's round border as ops.hip runs it: + Q, to Jacobian, two doublings, back, + Q (y through
    # cond_negate1 with neg false), to Jacobian
    xa = xyzz_add_affine(_xyzz_lift(c), NW, NW)
    j = xyzz_to_jacobian(xa)
    j = m.jpt_double(*m.jpt_double(*j))
    xa = xyzz_add_affine(xyzz_from_jacobian(j), NW, cond_negate1(NW, False))
    xyzz_to_jacobian(xa)


@functools.lru_cache(maxsize=None)
def _pt29q_operand(role, code):
    """PT29Q_*: cn = normalize_weak(c); P = (a cn : b cn : cn), Q = (d cn : e cn : cn); with c = 0 (the identity
    for P) Q = (normalize_weak(d), normalize_weak(e), 1).  Whether one operand at `code` passes its own steps."""
    x = lazy_bound(code)
    if role == "c":
        return _accepts(normalize_weak.body, x)
    ok = _accepts(lambda v: mul.body(v, NW), x)
    return ok and (role == "ab" or _accepts(normalize_weak.body, x))


@functools.lru_cache(maxsize=None)
def _pt29q_formulas():
    # every lane's coordinate is then a product, a weakly normalised value or 1 (COORD): the chained formulas
    return _accepts(lambda q: (ptq_add(q, q), ptq_double(q)), Quad([COORD] * 4))


def _pt29q(c):
    roles = ("ab", "ab", "c", "de", "de")
    assert all(_pt29q_operand(r, k) for r, k in zip(roles, c)) and _pt29q_formulas()


def _jac_nolift(c):
    # JDBL / JADD with bit 3 of c's code: P = (a, b, 1) as the lazy forms are, Q = (d, e) canonical
    x, y = lazy_bound(c[0]), lazy_bound(c[1])
    m.jpt_double(x, y, one.body())
    m.jpt_add_affine(x, y, one.body(), CANON, CANON)


# op -> (operands whose code the model decides, check)
BUDGET_FORMS = {
    "HP_JADD_NOLIFT": (2, _jac_nolift),
    "HP_AFF_DBL": (2, _aff_dbl),
    "HP_AFF_ADD": (4, _aff_add),
    "HP_PT29_ADD_MIXED": (2, _pt29_add_mixed),
    "HP_XYZZ_ADD": (3, _xyzz_add),
    "HP_XYZZ_ROUND": (3, _xyzz_round),
    "HP_PT29Q": (5, _pt29q),
}
# the maximal codes, pinned: a model change that moves them has to move these too
EXPECTED_BUDGETS = {
    "HP_JADD_NOLIFT": [(0, 1), (0, 4)],
    "HP_AFF_DBL": [(0, 0)],
    "HP_AFF_ADD": [(0, 0, 0, 7)],
    "HP_PT29_ADD_MIXED": [(0, 1), (0, 4), (1, 0), (4, 0)],
    "HP_XYZZ_ADD": [(7, 7, 1), (7, 7, 4)],
    "HP_XYZZ_ROUND": [(7, 7, 1), (7, 7, 4)],
    "HP_PT29Q": [(7, 7, 7, 7, 7)],
}
CODES = range(8)


def _accepts(check, arg):
    try:
        check(arg)
        return True
    except AssertionError:
        return False


def _above(c):
    """the codes one step above c: one more multiple of p, or the borrow spread added"""
    out = []
    if (c & 3) < 3:
        out.append(c + 1)
    if not c & 4:
        out.append(c | 4)
    return out


@functools.lru_cache(maxsize=None)
def max_codes(op):
    """the maximal code tuples (no operand can take one step more) the model accepts for `op`"""
    n, check = BUDGET_FORMS[op]
    ok = {t for t in itertools.product(CODES, repeat=n) if _accepts(check, t)}
    return sorted(t for t in ok if not any(t[:i] + (u,) + t[i + 1:] in ok for i in range(n) for u in _above(t[i])))


@pytest.mark.parametrize("op", sorted(BUDGET_FORMS))
def test_lazy_budgets(op):
    n, check = BUDGET_FORMS[op]
    tops = max_codes(op)
    assert tops == EXPECTED_BUDGETS[op]
    assert _accepts(check, (0,) * n) and all(_accepts(check, t) for t in tops)
    for t in tops:                                   # one step more on any operand is rejected
        for i in range(n):
            for u in _above(t[i]):
                assert not _accepts(check, t[:i] + (u,) + t[i + 1:])
