"""The affine formulas of aff29.h (the wide joint tables' odd multiples and lead points, keyed.hip) and the lazy 9x29 point
formulas of the multiscalar kernels, run on the device at exactly the lazy-operand budgets the interval model
(test_fe29_formulas_model.py) proves, against big-integer affine arithmetic (tests/pyref.py).

The affine formulas contain no curve constant, so any (x, y) with y != 0 is a point of y^2 = x^3 + b for b = y^2 - x^3:
coordinates with near-maximal canonical limbs (x just below p, every 29-bit limb all ones) are points of such curves.
"""
import random

import numpy as np
import pytest

import pyref as R
import test_fe29_formulas_model as fm

pytestmark = pytest.mark.gpu

P = R.P
M = (1 << 29) - 1
ALL_ONES = sum(M << (29 * i) for i in range(8)) + (((1 << 24) - 2) << 232)    # limbs 0..7 all ones, below p
assert ALL_ONES < P


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    import secp256k1_voi_amd as S
    return S.Engine(0)


def b32(v):
    return (v % P).to_bytes(32, "big")


def ints(a):
    return [int.from_bytes(bytes(x), "big") for x in np.asarray(a)]


def lazy(*codes):
    v = 0
    for j, c in enumerate(codes):
        v |= c << (4 * j)
    return v


def edge_values(rnd):
    return [P - 1, P - 2, P - 977, ALL_ONES, ALL_ONES - 1, 2**255, M, 2**232 - 1, 1, 2] + [rnd.randrange(1, P) for _ in range(6)]


def affine_points(rnd, count):
    """points of assorted curves y^2 = x^3 + b: edge-valued coordinates paired with each other, then random ones"""
    ev = edge_values(rnd)
    pts = [(x, y) for x in ev for y in ev if y % P]
    pts += [(rnd.randrange(P), rnd.randrange(1, P)) for _ in range(count)]
    return pts


def secp_points(rnd, count):
    """secp256k1 points, among them ones with near-maximal limbs (x lifted from values just below p and all-ones limbs)"""
    pts = []
    for base in (P - 1, ALL_ONES):
        x = base
        while len(pts) < (2 if base == P - 1 else 4):
            y = R.sqrt_p((x ** 3 + 7) % P)
            if y is not None and (y * y - x ** 3 - 7) % P == 0:
                pts += [(x, y), (x, P - y)]
            x -= 1
    k = rnd.randrange(1, R.N)
    q = R.mul(k, R.G)
    d = R.mul(rnd.randrange(1, R.N), R.G)
    while len(pts) < count:
        pts.append(q)
        q = R.add(q, d)
    return pts


def double_ref(p, k):
    for _ in range(k):
        p = R.add(p, p)
    return p


def add_ref(p, q, k):
    for _ in range(k):
        p = R.add(p, q)
    return p


def run_aff(eng, op, cols, codes, reps):
    import secp256k1_voi_amd as S
    x, y, flag = eng.fp_op_batch_ex(getattr(S, op), cols, lazy(*codes) | reps << 20)
    assert all(flag)
    return list(zip(ints(x), ints(y)))


@pytest.mark.parametrize("codes", fm.max_codes("HP_AFF_DBL"))
@pytest.mark.parametrize("reps", [1, 3, 9])
def test_aff_double(eng, codes, reps):
    """aff_double on points of many curves, chained as k_ksw_odd / k_ksw_lead do (2^k Q)."""
    pts = affine_points(random.Random(10 + reps), 300)
    got = run_aff(eng, "HP_AFF_DBL", [[b32(p[0]) for p in pts], [b32(p[1]) for p in pts]], codes, reps)
    for p, g in zip(pts, got):
        e = double_ref(p, reps)
        if e is not None:
            assert g == e, (p, reps)


@pytest.mark.parametrize("codes", fm.max_codes("HP_AFF_ADD") + [(0, 0, 0, 0)])
@pytest.mark.parametrize("reps", [1, 15])
def test_aff_add_odd_multiples(eng, codes, reps):
    """aff_add as k_ksw_odd chains it: B, B + 2B, B + 2 (2B), ... ((2a+1) B), on secp256k1 and on other curves."""
    rnd = random.Random(20 + reps)
    bs = secp_points(rnd, 40) + affine_points(rnd, 200)
    ds = [R.add(b, b) for b in bs]
    keep = [i for i, d in enumerate(ds) if d is not None and d[0] != bs[i][0]]
    bs, ds = [bs[i] for i in keep], [ds[i] for i in keep]
    cols = [[b32(b[0]) for b in bs], [b32(b[1]) for b in bs], [b32(d[0]) for d in ds], [b32(d[1]) for d in ds]]
    got = run_aff(eng, "HP_AFF_ADD", cols, codes, reps)
    for b, d, g in zip(bs, ds, got):
        e = add_ref(b, d, reps)
        if e is not None:
            assert g == e, (b, reps)


def test_aff_add_generic_pairs(eng):
    """aff_add of unrelated points (x1 != x2), the joint tables' shape: edge-valued x1, x2 and y1, y2 of one curve or not."""
    rnd = random.Random(30)
    ps = affine_points(rnd, 150)
    qs = ps[1:] + ps[:1]
    keep = [i for i in range(len(ps)) if ps[i][0] != qs[i][0]]
    ps, qs = [ps[i] for i in keep], [qs[i] for i in keep]
    cols = [[b32(p[0]) for p in ps], [b32(p[1]) for p in ps], [b32(q[0]) for q in qs], [b32(q[1]) for q in qs]]
    for codes in fm.max_codes("HP_AFF_ADD"):
        got = run_aff(eng, "HP_AFF_ADD", cols, codes, 1)
        for p, q, g in zip(ps, qs, got):
            assert g == R.add(p, q), (p, q, codes)


def _lifted_cols(rnd, pts, qs):
    z = [rnd.randrange(1, P) for _ in pts]
    z[:4] = [1, P - 1, ALL_ONES, 2]
    return [[b32(p[0]) for p in pts], [b32(p[1]) for p in pts], [b32(v) for v in z],
            [b32(q[0]) for q in qs], [b32(q[1]) for q in qs]]


@pytest.mark.parametrize("codes", fm.max_codes("HP_XYZZ_ADD"))
def test_xyzz_at_model_budget(eng, codes):
    """xyzz29_add_affine with P lifted from operands at the largest lazy codes the model accepts (a, b, c), on points
    with near-maximal limbs.  (The harness weakly normalises Q: the negated bucket-pass addend, 2p - y limb by limb,
    is bounded by the model only.)"""
    import secp256k1_voi_amd as S
    rnd = random.Random(40 + sum(codes))
    pts = secp_points(rnd, 120)
    qs = pts[3:] + pts[:3]
    cols = _lifted_cols(rnd, pts, qs)
    x, y, flag = eng.fp_op_batch_ex(S.HP_XYZZ_ADD, cols, lazy(*codes))
    for p, q, xi, yi, f in zip(pts, qs, ints(x), ints(y), flag):
        assert f == 1 and (xi, yi) == R.add(p, q)


@pytest.mark.parametrize("codes", fm.max_codes("HP_XYZZ_ROUND"))
def test_xyzz_round_at_model_budget(eng, codes):
    """The keyed ladder's round border (XYZZ addition, to Jacobian, two doublings, back, addition, to Jacobian) at the
    model's largest codes for the round, on points with near-maximal limbs."""
    import secp256k1_voi_amd as S
    rnd = random.Random(45 + sum(codes))
    pts = secp_points(rnd, 120)
    qs = pts[3:] + pts[:3]
    cols = _lifted_cols(rnd, pts, qs)
    x, y, flag = eng.fp_op_batch_ex(S.HP_XYZZ_ROUND, cols, lazy(*codes))
    for p, q, xi, yi, f in zip(pts, qs, ints(x), ints(y), flag):
        s = R.add(p, q)
        s4 = R.add(R.add(s, s), R.add(s, s))
        assert f == 1 and (xi, yi) == R.add(s4, q)


@pytest.mark.parametrize("codes", fm.max_codes("HP_PT29_ADD_MIXED"))
def test_pt29_add_mixed_at_model_budget(eng, codes):
    """pt29_add_mixed (the redo path, msm_piece) with the affine addend's coordinates at the model's largest codes."""
    import secp256k1_voi_amd as S
    rnd = random.Random(50 + sum(codes))
    pts = secp_points(rnd, 120)
    qs = pts[5:] + pts[:5]
    cols = _lifted_cols(rnd, pts, qs)
    x, y, flag = eng.fp_op_batch_ex(S.HP_PT29_ADD_MIXED, cols, lazy(0, 0, 0, *codes))
    for p, q, xi, yi, f in zip(pts, qs, ints(x), ints(y), flag):
        e = R.add(p, q)
        assert (f == 0) if e is None else (f == 1 and (xi, yi) == e)


@pytest.mark.parametrize("codes", fm.max_codes("HP_JADD_NOLIFT"))
def test_jacobian_no_lift_high_limbs(eng, codes):
    """jpt29_double / jpt29_add_affine with P = (a, b, 1) taken in its lazy form (bit 3 of c's code: no lift) at the model's
    largest codes, on points with near-maximal canonical limbs."""
    import secp256k1_voi_amd as S
    rnd = random.Random(60 + sum(codes))
    pts = secp_points(rnd, 100)
    qs = pts[7:] + pts[:7]
    cols = _lifted_cols(rnd, pts, qs)
    x, y, flag = eng.fp_op_batch_ex(S.HP_JDBL, cols, lazy(codes[0], codes[1], 8))
    for p, xi, yi, f in zip(pts, ints(x), ints(y), flag):
        assert f == 1 and (xi, yi) == R.add(p, p)
    x, y, flag = eng.fp_op_batch_ex(S.HP_JADD, cols, lazy(codes[0], codes[1], 8))
    for p, q, xi, yi, f in zip(pts, qs, ints(x), ints(y), flag):
        assert f == 1 and (xi, yi) == R.add(p, q)


@pytest.mark.parametrize("codes", fm.max_codes("HP_PT29Q"))
@pytest.mark.parametrize("reps", [1, 6])
def test_pt29q_chains_high_limbs(eng, codes, reps):
    """pt29q_add / pt29q_double (the multiscalar tail) chained on points with near-maximal limbs, every operand at the
    model's largest code; c = 0 on one row makes P the identity (Q then taken as normalize_weak(d), normalize_weak(e))."""
    import secp256k1_voi_amd as S
    rnd = random.Random(70 + reps)
    pts = secp_points(rnd, 80)
    qs = pts[2:] + pts[:2]
    cols = _lifted_cols(rnd, pts, qs)
    cols[2][4] = b32(0)
    starts = [None if i == 4 else p for i, p in enumerate(pts)]
    x, y, flag = eng.fp_op_batch_ex(S.HP_PT29Q_ADD, cols, lazy(*codes) | reps << 20)
    for p, q, xi, yi, f in zip(starts, qs, ints(x), ints(y), flag):
        e = add_ref(p, q, reps)
        assert (f == 0) if e is None else (f == 1 and (xi, yi) == e)
    x, y, flag = eng.fp_op_batch_ex(S.HP_PT29Q_DBL, cols, lazy(*codes) | reps << 20)
    for p, xi, yi, f in zip(starts, ints(x), ints(y), flag):
        e = double_ref(p, reps)
        assert (f == 0) if e is None else (f == 1 and (xi, yi) == e)
