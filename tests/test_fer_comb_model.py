"""The wave-per-signature ladder over a comb key table (csrc/fe29r.h: pt29r_pair_from_iso; small_call.hip: row_ladder_comb) on the
lane-level model tests/fer_comb_model.py: the entry conversion against big-integer arithmetic, limb bounds at the top of what
the ladder feeds each formula, and the whole key part - column 18 as a pair sum, 18 rounds of doubling and two additions -
against +-k1 Q +- k2 lambda(Q) for random half scalars and the recoding's corners.  No GPU; the compiled functions run in
tests/test_gpu_keyset_comb_row.py."""
import random

import pytest

import fer_comb_model as C
import fer_model as F
import pyref as R
import test_comb_model as cm
import test_glv_odd_model as glv
from test_fer_model import BOUND1, affine, lazy

P, N = F.P, R.N


def to_iso(pt, w):
    return pt[0] * w * w % P, pt[1] * pow(w, 3, P) % P


def top(u):
    return F.lane_const(lambda j, r: u * BOUND1[j] if j <= 8 else 0)


def one_unit(*regs):
    return all(c[l] <= BOUND1[l & 15] if (l & 15) <= 8 else c[l] == 0 for c in regs for l in range(F.LANES))


def two_units(c):
    return all(c[l] <= 2 * BOUND1[l & 15] if (l & 15) <= 8 else c[l] == 0 for l in range(F.LANES))


def test_pair_from_iso_is_the_point_of_secp256k1():
    """(x, y) on y^2 = x^3 + 7 W^6 -> (x W : y : W^3) is the point (x / W^2, y / W^3) of secp256k1: both halves of the layer,
    random W and the two ends W = 1 and W = p - 1, y with one and two units passed through untouched"""
    rnd = random.Random(2101)
    for it in range(24):
        w = (1, P - 1)[it] if it < 2 else rnd.randrange(2, P)
        p, q = R.mul(rnd.randrange(1, N), R.G), R.mul(rnd.randrange(1, N), R.G)
        (x1, y1), (x2, y2) = to_iso(p, w), to_iso(q, w)
        assert (y1 * y1 - x1 ** 3 - 7 * pow(w, 6, P)) % P == 0
        wv, w3 = C.comb_consts(lazy(w, rnd))
        assert F.fer_value(w3) % P == pow(w, 3, P) and one_unit(w3)
        Y1, Y2 = lazy(y1, rnd, 1 + it % 2), lazy(y2, rnd, 1 + (it // 2) % 2)
        e1, e2 = C.pair_from_iso(lazy(x1, rnd), Y1, lazy(x2, rnd), Y2, wv, w3)
        assert affine(*e1) == p and affine(*e2) == q
        assert e1[1] is Y1 and e2[1] is Y2 and e1[2] is w3 and e2[2] is w3 and one_unit(e1[0], e2[0])
        # ... and what the ladder does with them: the complete sum, P + P and P - P included
        assert affine(*F.ptr_add(e1, e2)) == R.add(p, q)
        assert affine(*F.ptr_add(e1, e1)) == R.add(p, p)
        n1 = (e1[0], F.fer_negate(F.fer_norm(e1[1]), 1), e1[2])
        assert affine(*F.ptr_add(e1, n1)) is None


def test_limb_bounds_of_a_round():
    """Every operand at the TOP of its budget - x, W, W^3 and the accumulator's X, Z one unit; y two units into the doubling
    (what a doubling leaves) and into both additions (a doubling's output on one side, a negated entry on the other): the
    model asserts each 32- / 64-bit width inside its products, so running the round is the proof; what comes out is one unit
    (the doubling's Y: two), so the bound holds along the ladder."""
    w, w3 = C.comb_consts(top(1))
    assert one_unit(w3)
    yneg = F.fer_negate(top(1), 1)                           # a negated entry: within two units
    assert two_units(yneg)
    for y in (top(2), yneg, top(1)):
        e1, e2 = C.pair_from_iso(top(1), y, top(1), y, w, w3)
        assert one_unit(e1[0], e2[0], e1[2], e2[2])
        assert one_unit(*F.ptr_add(e1, e2))                  # column 18
        acc = (top(1), top(2), top(1))
        d = F.ptr_double(*acc)
        assert one_unit(d[0], d[2]) and two_units(d[1])
        a1 = F.ptr_add((d[0], top(2), d[2]), e1)
        assert one_unit(*a1)
        assert one_unit(*F.ptr_add((a1[0], top(2), a1[2]), e2))
    # the whole key part on a table whose every word is at the top of one unit (no point: only the widths are looked at)
    acc = C.row_ladder_comb_key_part(lambda entry, which: top(1), w, w3, 2 ** 129 - 1, True, 1, False)
    assert one_unit(*acc)


@pytest.fixture(scope="module")
def key():
    rnd = random.Random(2102)
    q = R.mul(rnd.randrange(1, N), R.G)
    return q, [R.mul(cm.entry_scalar(i), q) for i in range(64)]      # E[idx] = B_6 + sum_{t<6} (2 idx_t - 1) B_t, B_t = 2^(19 t) Q


def loader(entries, w, rnd):
    """ke_row_load over the key's table on the curve isomorphic by w: x, y and beta x of an entry, one unit each"""
    iso = [to_iso(e, w) for e in entries]
    return lambda entry, which: lazy((iso[entry][0], iso[entry][1], iso[entry][0] * R.BETA % P)[which], rnd)


def run(entries, w, rnd, k1, neg1, k2, neg2, flip=False):
    wv, w3 = C.comb_consts(lazy(w, rnd))
    return affine(*C.row_ladder_comb_key_part(loader(entries, w, rnd), wv, w3, k1, neg1, k2, neg2, flip))


def want(q, k1, neg1, k2, neg2):
    return R.mul(((-k1 if neg1 else k1) + (-k2 if neg2 else k2) * R.LAMBDA) % N, q)


# 1: every tooth all zeros (a = 0); 2^129 - 1: every bit the half scalar has set; 2^128 + 1: only the top bit of a; the column
# patterns: one tooth all ones, one column all ones
CORNERS = [1, 2 ** 128 + 1, 2 ** 129 - 1, 3, 2 ** 128 - 1, (2 ** 19 - 1 << 1) + 1, sum(2 ** (19 * t + 1) for t in range(7)) + 1,
           (2 ** 128 - 2 ** 114 << 1) + 1]


def test_teeth_and_columns():
    assert C.teeth_of(1) == [0] * 6 + [1 << 18] and C.teeth_of(2 ** 129 - 1) == [2 ** 19 - 1] * 6 + [(1 << 18) | (2 ** 14 - 1)]
    assert C.teeth_of(2 ** 128 + 1)[6] == (1 << 18) | (1 << 13)
    for k in CORNERS + [random.Random(2103).randrange(1 << 129) | 1 for _ in range(200)]:
        assert (k >> 1) | 1 << C.LEAD_BIT == sum(t << (19 * i) for i, t in enumerate(C.teeth_of(k)))
        acc = 0
        for j in range(18, -1, -1):
            e, neg = C.column_of(C.teeth_of(k), j)
            acc = 2 * acc + (-cm.entry_scalar(e) if neg else cm.entry_scalar(e))
        assert acc == k, hex(k)
    # column 18 is never negative: the lead is its top tooth's bit
    assert all(not C.column_of(C.teeth_of(k), 18)[1] for k in CORNERS)


def test_ladder_corners_signs_and_flip(key):
    """+-k1 Q +- k2 lambda(Q) for the corner half scalars against each other, every pair of sign flags, and `flip`"""
    q, entries = key
    rnd = random.Random(2104)
    w = rnd.randrange(2, P)
    halves = [(CORNERS[i], CORNERS[(i * 3 + 1) % len(CORNERS)]) for i in range(len(CORNERS))]
    for i, (k1, k2) in enumerate(halves):
        for n1, n2 in ((False, False), (True, False), (False, True), (True, True)) if i < 3 else (((i & 1) != 0, (i & 2) != 0),):
            for flip in (False, True):
                got = run(entries, w, rnd, k1, n1, k2, n2, flip)
                assert got == want(q, k1, n1 != flip, k2, n2 != flip), (hex(k1), n1, hex(k2), n2, flip)


def test_ladder_random_halves_and_both_ends_of_w(key):
    q, entries = key
    rnd = random.Random(2105)
    for it in range(8):
        w = (1, P - 1)[it & 1] if it < 4 else rnd.randrange(2, P)
        k1, k2 = rnd.randrange(1 << 129) | 1, rnd.randrange(1 << 129) | 1
        n1, n2 = rnd.random() < 0.5, rnd.random() < 0.5
        assert run(entries, w, rnd, k1, n1, k2, n2) == want(q, k1, n1, k2, n2), (it, hex(k1), hex(k2))


def test_ladder_on_the_chosen_scalars(key):
    """u2 Q for the scalars tests/test_gpu_comb.py chooses (the teeth, the lead, a full column, the boundary halves), split as
    the device splits them (test_glv_odd_model)"""
    import test_gpu_comb as TC
    q, entries = key
    rnd = random.Random(2106)
    w = rnd.randrange(2, P)
    for u2 in TC.chosen_u2():
        k1, k2 = glv.make_odd(*glv.split_reference(u2))
        assert run(entries, w, rnd, abs(k1), k1 < 0, abs(k2), k2 < 0) == R.mul(u2, q), hex(u2)


def test_equal_and_opposite_entries_in_a_column_are_no_exception(key):
    """k1 = k2 with lambda's image replaced by the point itself (beta x := x): every column adds E to E, or E to -E under
    opposite signs - the complete formulas take both, where the lane ladder ends on its worklist"""
    q, entries = key
    rnd = random.Random(2107)
    w = rnd.randrange(2, P)
    iso = [to_iso(e, w) for e in entries]
    load = lambda entry, which: lazy(iso[entry][1 if which == 1 else 0], rnd)
    wv, w3 = C.comb_consts(lazy(w, rnd))
    k = rnd.randrange(1 << 129) | 1
    assert affine(*C.row_ladder_comb_key_part(load, wv, w3, k, False, k, False)) == R.mul(2 * k % N, q)
    assert affine(*C.row_ladder_comb_key_part(load, wv, w3, k, False, k, True)) is None


def test_layers_of_the_key_part(key, monkeypatch):
    """37 additions of 3 layers, 18 doublings of 2, 19 conversions: 166 row products (row_ladder_keyset: 64 x 4 + 1 = 257)"""
    q, entries = key
    rnd = random.Random(2108)
    calls = []
    real = F.fer_mulsum
    monkeypatch.setattr(F, "fer_mulsum", lambda pairs, addend=None: (calls.append(len(pairs)), real(pairs, addend))[1])
    run(entries, 5, rnd, 3, False, 5, True)
    assert len(calls) - 2 == 37 * 3 + 18 * 2 + 19 == 166          # (- 2: W^3, formed in front of the ladder)
