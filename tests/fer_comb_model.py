"""Lane-level model of pt29r_pair_from_iso (csrc/fe29r.h) and of the key part of row_ladder_comb (small_call.hip), in the style of
tests/fer_b3_model.py and on top of tests/fer_model.py: the wave-per-signature ladder over a COMB key table.  An entry of
such a table is an affine point (x, y) of the key's isomorphic curve y^2 = x^3 + 7 W^6; (x W : y : W^3) is that point on
secp256k1 itself, so the ladder doubles and adds there (fer_model.ptr_double / ptr_add) and carries no per-key constant.  The
device code is a transcription of these functions; every width it relies on is asserted inside fer_model's products, so
running the model at the top of the lazy bounds is the overflow proof of the schedule."""
import fer_model as F

TEETH, SPACING = 7, 19
LEAD_BIT = TEETH * SPACING - 1          # bit 132 of a' = bit 18 of the top tooth


def comb_consts(w):
    """W (one unit, all rows) -> W, W^3 as the kernels form them once per signature (small_call.hip: row_comb_iso_of)"""
    return w, F.fer_mul(F.fer_mul(w, w), w)


def pair_from_iso(x1, y1, x2, y2, w, w3):
    """the two entries of a column, (x1, y1) and (x2, y2) affine on y^2 = x^3 + 7 W^6 -> (x W : y : W^3) each, one layer:
    x1 W in rows 0, 1 and x2 W in rows 2, 3.  In: x, W, W^3 one unit, y up to two (untouched); out the same."""
    Mv = F.fer_mul(F.sel((x1, x1, x2, x2)), w)                                   # x1 W | x1 W | x2 W | x2 W
    X1, X2 = F.permlane32_swap(Mv, Mv)
    return (X1, y1, w3), (X2, y2, w3)


def teeth_of(k):
    """the seven teeth of a' = (k >> 1) | 2^132 for an odd half scalar k < 2^129, cut from the words of k as the kernel cuts them"""
    assert k & 1 and 0 < k < 1 << 129
    words = [(k >> (32 * i)) & 0xFFFFFFFF for i in range(5)]
    teeth = []
    for t in range(TEETH):
        bit = SPACING * t + 1
        limb, sh = bit >> 5, bit & 31
        v = words[limb] >> sh
        if sh > 32 - SPACING:
            v |= (words[limb + 1] << (32 - sh)) & 0xFFFFFFFF
        teeth.append(v & ((1 << SPACING) - 1))
    teeth[TEETH - 1] |= 1 << (SPACING - 1)
    return teeth


def column_of(teeth, j):
    """(entry, negative) of column j: the 7-bit index w, its top bit the sign"""
    w = 0
    for t in range(TEETH):
        w |= ((teeth[t] >> j) & 1) << t
    top = bool(w & 64)
    return (w if top else ~w) & 63, not top


def row_ladder_comb_key_part(load, w, w3, k1, neg1, k2, neg2, flip=False):
    """The key part of row_ladder_comb: (+-k1) Q + (+-k2) lambda(Q) as (X, Y, Z) on secp256k1.  load(entry, which) is
    ke_row_load: the register holding x (0), y (1) or beta x (2) of table entry `entry`, one unit.  Column 18 starts the
    accumulator as the sum of its two entries; rounds 17..0 double, add E1, add phi(E2)."""
    neg1, neg2 = neg1 != flip, neg2 != flip
    t1, t2 = teeth_of(k1), teeth_of(k2)

    def entries(j):
        (i1, m1), (i2, m2) = column_of(t1, j), column_of(t2, j)
        y1, y2 = load(i1, 1), load(i2, 1)
        if neg1 != m1:
            y1 = F.fer_negate(y1, 1)                                             # [2]: the addition normalises y
        if neg2 != m2:
            y2 = F.fer_negate(y2, 1)
        return pair_from_iso(load(i1, 0), y1, load(i2, 2), y2, w, w3)
    e1, e2 = entries(SPACING - 1)
    acc = F.ptr_add(e1, e2)
    for j in range(SPACING - 2, -1, -1):
        acc = F.ptr_double(*acc)
        e1, e2 = entries(j)
        acc = F.ptr_add(acc, e1)
        acc = F.ptr_add(acc, e2)
    return acc
