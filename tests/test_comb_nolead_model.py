"""Model of the comb ladder without the lead point (comb_ladder.hip: k_verify_comb), without a GPU.

k_verify_fast<MODE_.._COMB> recodes an odd half scalar k < 2^129 as 2^133 + sum_{i<133} (2 a_i - 1) 2^i with a = k >> 1 and
starts from the lead pair 2^133 Q.  With a' = a | 2^132 the same 133 digits sum to k by themselves:
sum (2 a'_i - 1) 2^i = 2 a' - (2^133 - 1) = k.  Only bit 18 of the top tooth changes, column 18 then STARTS the
accumulator - its pair sum is a Jacobian point as it stands - and rounds 17 .. 0 run as they did.

  * the identity on integers, and the digits the kernel forms against test_comb_model.comb_digits;
  * the whole ladder on the limb schedule over a table built by the model, both signs of both halves, against pyref;
  * interval bounds of the peeled round in the units of fe29.h;
  * a drift guard on comb_ladder.hip: the loop's column is the existing block's, the peeled round has the pair sum only;
  * two mutations the value model rejects: bit 18 not set, the sign of t.ny in the peeled round.
"""
import random
import re

import pytest

import pyref as R
import test_comb_model as cm
import test_comb_pair_model as cp
import test_fe29_formulas_model as fm
import test_fe29_model as m
from test_fe29_formulas_model import COORD, Y2, cond_negate1, le, within
from test_fe29_model import P

N = R.N
TEETH, SPACING, LEN = cm.TEETH, cm.SPACING, cm.LEN
LEAD_BIT = LEN - 1                                   # bit 132 of a' = bit 18 of the top tooth
BOUNDARY = [1, 3, 2**128 - 1, 2**128 + 1, 2**129 - 1]


def odd_halves():
    rng = random.Random(2020)
    return BOUNDARY + [rng.randrange(1 << 129) | 1 for _ in range(1000)]


# ==== the recoding ======================================================================================================
def nolead_digits(k, lead_bit=True):
    """[(entry, negative)] of the rounds j = 18 .. 0 as k_verify_comb forms them: the teeth of test_comb_model.comb_digits from
    the words of k, bit 18 of the top tooth set, bit j of each, the top tooth's bit as the sign"""
    assert k & 1 and 0 < k < 1 << 129
    words = [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    teeth = []
    for t in range(TEETH):
        bit = SPACING * t + 1
        limb, sh = bit >> 5, bit & 31
        v = words[limb] >> sh
        if sh > 32 - SPACING:
            v |= (words[limb + 1] << (32 - sh)) & 0xFFFFFFFF
        teeth.append(v & ((1 << SPACING) - 1))
    if lead_bit:
        teeth[TEETH - 1] |= 1 << (SPACING - 1)
    out = []
    for j in range(SPACING - 1, -1, -1):
        w = 0
        for t in range(TEETH):
            w |= ((teeth[t] >> j) & 1) << t
        top = bool(w & 64)
        out.append(((w if top else ~w) & 63, not top))
    return out


def test_the_kernel_sets_the_bit_where_the_model_does():
    src = fm.body_of("comb_ladder.hip", "k_verify_comb")
    assert src.count("t1[G::TEETH - 1] |= 1u << (G::SPACING - 1);") == 1 and src.count("t2[G::TEETH - 1] |= 1u << (G::SPACING - 1);") == 1
    # ... behind the teeth's masks and in front of the columns' cut
    assert src.index("t2[t] = v2 & ((1u << G::SPACING) - 1u);") < src.index("t1[G::TEETH - 1] |=") < src.index("cols[j][threadIdx.x] = w;")
    assert (TEETH - 1) * SPACING + SPACING - 1 == LEAD_BIT == 132


def test_identity_on_integers():
    """sum_{i<133} (2 a'_i - 1) 2^i = k for a' = (k >> 1) | 2^132: no lead term"""
    for k in odd_halves():
        a = k >> 1
        assert a < 1 << 128                                        # so bit 132 is free
        ap = a | (1 << LEAD_BIT)
        assert sum((2 * ((ap >> i) & 1) - 1) << i for i in range(LEN)) == k, hex(k)
        assert 2 * ap - ((1 << LEN) - 1) == k
        # the existing recoding, for comparison: the same sum over a, plus the lead 2^133
        assert (1 << LEN) + sum((2 * ((a >> i) & 1) - 1) << i for i in range(LEN)) == k


def test_digits_sum_to_the_scalar_without_a_lead():
    for k in odd_halves():
        acc = 0
        for r, (entry, negative) in enumerate(nolead_digits(k)):
            if r:
                acc *= 2
            acc += -cm.entry_scalar(entry) if negative else cm.entry_scalar(entry)
        assert acc == k, hex(k)


def test_digits_are_the_existing_ones_but_for_bit_18_of_the_top_tooth():
    for k in odd_halves():
        old, new = cm.comb_digits(k), nolead_digits(k)
        assert old[1:] == new[1:], hex(k)                          # columns 17 .. 0
        # column 18: the top tooth was negative there (a has 128 bits), now it is positive: the complemented entry
        (e_old, neg_old), (e_new, neg_new) = old[0], new[0]
        assert neg_old and not neg_new and e_new == ~e_old & 63
        # the top tooth's constant bits: bits 128 .. 131 of a are 0 (columns 14 .. 17: negative), bit 132 of a' is 1
        assert all(new[SPACING - 1 - j][1] for j in (14, 15, 16, 17)) and not new[0][1]
        # ... and the two columns differ by the lead: +E[e_new] - (-E[e_old]) = 2^115, times 2^18
        assert cm.entry_scalar(e_new) + cm.entry_scalar(e_old) == 2 << (6 * SPACING) == 1 << cm.LEAD_LOG2


# ==== the ladder on the limb schedule =====================================================================================
def first_round_int(e1, e2, n1, n2, flip_ny=False):
    """the peeled round: acc = (t.x, +-t.ny, t.h) from the pair sum, E2 with its sign relative to E1's"""
    t = cp.pair_sum_int(e1[0], e1[1], e2[0], cp.cond_negate1_int(e2[1], n1 != n2))
    return t[0], cp.cond_negate1_int(t[1], (not n1) != flip_ny), t[2]


def ladder_int(entries, k1, k2, lead_bit=True, flip_ny=False):
    """k_verify_comb's ladder on the limb schedule: the peeled round 18, then 18 x (doubling, column); Z is over the table's W"""
    neg1, neg2 = k1 < 0, k2 < 0
    d1, d2 = nolead_digits(abs(k1), lead_bit), nolead_digits(abs(k2), lead_bit)

    def pair(r):
        (i1, m1), (i2, m2) = d1[r], d2[r]
        e1, e2 = entries[i1], entries[i2]
        return (m.from_int(e1[0]), m.from_int(e1[1])), (m.from_int(e2[2]), m.from_int(e2[1])), neg1 != m1, neg2 != m2
    acc = first_round_int(*pair(0), flip_ny=flip_ny)
    assert all(x <= 2 * m.M + (1 << 21) for v in acc for x in v)
    for r in range(1, SPACING):
        acc = cp.double_int(acc)
        acc = cp.column_int(acc, *pair(r))
        assert all(x <= 2 * m.M + (1 << 21) for v in acc for x in v)
    return acc


@pytest.fixture(scope="module")
def table():
    rng = random.Random(2021)
    d = rng.randrange(1, N)
    Q = R.mul(d, R.G)
    lead, pt, zac = cm.chain_comb(Q)
    entries, _lead_pair, W = cm.finish_comb(lead, pt, zac)        # (the lead pair is built and not read)
    return Q, entries, W


def _want(k1, k2, Q):
    return R.mul((k1 + k2 * R.LAMBDA) % N, Q)


HALVES = [(1, 1), (3, 2**128 + 1), (2**128 - 1, 3), (2**129 - 1, 2**129 - 1), (2**128 + 1, 1)]


def test_ladder_is_k1_Q_plus_k2_phi_Q_for_both_signs_of_both_halves(table):
    Q, entries, W = table
    rng = random.Random(2022)
    halves = HALVES + [(rng.randrange(1 << 129) | 1, rng.randrange(1 << 129) | 1) for _ in range(3)]
    for a, b in halves:
        for s1 in (1, -1):
            for s2 in (1, -1):
                k1, k2 = s1 * a, s2 * b
                assert cp._aff(ladder_int(entries, k1, k2), W) == _want(k1, k2, Q), (hex(a), hex(b), s1, s2)


def test_ladder_on_split_scalars(table):
    """u2 as the device splits it (test_glv_odd_model): the same result as the ladder with the lead point"""
    import test_glv_odd_model as glv
    Q, entries, W = table
    rng = random.Random(2023)
    for u2 in (1, 3, R.LAMBDA + 1, N - 1, rng.randrange(1, N)):
        k1, k2 = glv.make_odd(*glv.split_reference(u2))
        assert cp._aff(ladder_int(entries, k1, k2), W) == R.mul(u2, Q), hex(u2)


def test_equal_entries_in_the_first_round_leave_z_zero(table):
    """h = 0 in the peeled round: Z = 0 from the start, and it stays (the worklist's case)"""
    _, entries, _ = table
    e = entries[5]
    e1 = (m.from_int(e[0]), m.from_int(e[1]))
    acc = first_round_int(e1, e1, False, False)
    assert m.value(acc[2]) % P == 0
    acc = cp.double_int(acc)
    assert m.value(acc[2]) % P == 0
    e2 = entries[9]
    acc = cp.column_int(acc, e1, (m.from_int(e2[2]), m.from_int(e2[1])), False, True)
    assert m.value(acc[2]) % P == 0


# ==== the two mutations ====================================================================================================
def test_mutation_bit_18_not_set_is_rejected(table):
    Q, entries, W = table
    for a, b in HALVES[:3]:
        got = cp._aff(ladder_int(entries, a, -b, lead_bit=False), W)
        assert got != _want(a, -b, Q)
        # what it computes instead: both halves short of their lead 2^133, each with its sign
        assert got == _want(a - (1 << LEN), -(b - (1 << LEN)), Q)


def test_mutation_sign_of_ny_in_the_peeled_round_is_rejected(table):
    Q, entries, W = table
    for a, b in HALVES[:3]:
        for s1 in (1, -1):
            assert cp._aff(ladder_int(entries, s1 * a, b, flip_ny=True), W) != _want(s1 * a, b, Q)


# ==== interval bounds of the peeled round ==================================================================================
def first_round(x1, y1, x2, y2):
    """the peeled round's calls in the text's order: the pair sum of the two entries (E2's y through fe29_cond_negate1), its
    x, its ny through fe29_cond_negate1 and its h as the accumulator, into the doubling"""
    t = cp.pair_sum(x1, y1, x2, cond_negate1(y2))
    return t[0], cond_negate1(t[1]), t[2]


def test_bounds_of_the_peeled_round():
    x, y, z = first_round(COORD, COORD, COORD, COORD)
    assert le(x, COORD) and le(z, COORD)            # t.x [1], t.h [1] (weakly normalised)
    assert le(y, Y2)                                # +-t.ny: at most [2]
    assert within((x, y, z), cp.JPT_BOX)            # what jpt29_double takes: x [1], y [<= 2], z [1]
    d = m.jpt_double(x, y, z)
    assert within(d, cp.JPT_BOX)
    assert within(cp.column(d, COORD, COORD, COORD, COORD), cp.JPT_BOX)       # ... and round 17 takes the doubling's point
    with pytest.raises(AssertionError):
        first_round(COORD, Y2, COORD, COORD)        # y1 of two units: the pair sum's contract (test_comb_pair_model)


# ==== drift guard ===========================================================================================================
@pytest.fixture
def tracked(monkeypatch):
    monkeypatch.setattr(fm, "TRACKED", re.compile(fm.TRACKED.pattern.replace(r"(fe29_\w+", r"(fe29_\w+|coz29_\w+")))


def ladder_text():
    body = fm.body_of("comb_ladder.hip", "k_verify_comb")
    lo, hi = body.index("jpt29 acc;"), body.index("bool final_only")
    text = body[lo:hi]
    cut = text.index("for (int j = G::SPACING - 2; j >= 0; --j) {")
    loop_end = text.index("acc.z = fe29_mul(acc.z, ke_load(")
    return text[:cut], text[cut:loop_end], text[loop_end:]


def old_column_text():
    old = cp.comb_block_text()
    return old[old.index("for (int j = G::SPACING - 1;; --j) {"):old.index("if (j == 0) break;")]


def test_drift_guard_of_the_ladder(tracked):
    peeled, loop, tail = ladder_text()
    # the loop: one doubling, then the existing block's column, call for call and line for line
    old_col = old_column_text()
    assert fm.calls_in(loop) == ["jpt29_double"] + fm.calls_in(old_col)
    assert m.record(lambda *a: cp.column(*a), cp.JPT_BOX, COORD, COORD, COORD, COORD) == fm.calls_in(old_col)
    for line in ("coz29_pair_sum(x1, y1, x2, fe29_cond_negate1(y2, n1 != n2))", "acc = jpt29_rescale(acc, t.hh, t.hhh);",
                 "acc = jpt29_add_affine(acc, t.x, fe29_cond_negate1(t.ny, !n1));", "acc.z = fe29_mul(acc.z, t.h);",
                 "ke_load_xy(kt + (size_t)((top1 ? w1 : ~w1) & 63u) * 8, false, x1, y1);",
                 "ke_load_xy(kt + (size_t)((top2 ? w2 : ~w2) & 63u) * 8, true, x2, y2);",
                 "const bool n1 = neg1 != !top1, n2 = neg2 != !top2;"):
        assert line in loop and line in old_col, line
    assert loop.count("jpt29_double(") == 1 and loop.index("jpt29_double(") < loop.index("coz29_pair_sum(")
    # the peeled round: both lookups and the pair sum, nothing of the addition to an accumulator, and no lead lookup
    assert fm.calls_in(peeled) == m.record(first_round, COORD, COORD, COORD, COORD)
    assert peeled.count("coz29_pair_sum(") == 1 and peeled.count("ke_load_xy(") == 2
    assert "jpt29_rescale" not in peeled and "jpt29_add_affine" not in peeled and "fe29_mul" not in peeled
    assert "acc.x = t.x;" in peeled and "acc.y = fe29_cond_negate1(t.ny, !n1);" in peeled and "acc.z = t.h;" in peeled
    assert "cols[G::SPACING - 1][threadIdx.x]" in peeled
    # behind the loop: W
    assert fm.calls_in(tail) == ["fe29_mul"]
    whole = fm.body_of("comb_ladder.hip", "k_verify_comb")
    assert "LEAD" not in whole and whole.count("ke_load_xy(") == 4


def test_products_of_the_ladder():
    """526 -> 512: the first column's 20 products become the pair sum's 6"""
    with_lead = 19 * 20 + 18 * 7 + 1 + 16 + 3        # columns, doublings, W, the final Jacobian + Jacobian addition, the comparison
    assert with_lead == 526
    assert with_lead - (2 + 11 + 1) == 6 + 18 * 20 + 18 * 7 + 1 + 16 + 3 == 512


def test_routing_in_launch_ladder():
    body = fm.body_of("lane_kernels.hip", "launch_ladder")
    assert body.count("k_verify_comb<false><<<") == 1 and body.count("k_verify_comb<true><<<") == 1
    assert 'getenv("S2K_COMB_LEAD")' in body and "static" not in body[:body.index("switch (mode)")]      # read at every call
    assert "S2K_LADDER(MODE_ECDSA_COMB)" in body and "S2K_LADDER(MODE_SCHNORR_COMB)" in body             # the old instantiations stay
    # the only launches of the new kernel in the library
    for f in ("engine.hip", "lane_kernels.hip", "fallback.hip", "worklist.hip", "verify_fast.h", "ladder_ecdsa.hip", "ladder_schnorr.hip",
              "keyed.hip", "keyset.hip", "comb_ladder.hip"):
        assert fm.source(f).count("k_verify_comb<") == (2 if f == "lane_kernels.hip" else 2 if f == "comb_ladder.hip" else 0), f
