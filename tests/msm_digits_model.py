"""Big-integer model of what the bucket method of secp256k1_voi_amd/csrc/msm.hip does to a 128-bit magnitude before any point
is touched: msm_digit and msm_for_digits (the signed recoding: key = window * nb + |digit| - 1, sign, carry, the unsigned top
window that continues into an extra slot), msm_setup's choice of the window width from the term count, and the key range.
The endomorphism split in front of it is pointset_model.split.

classify() names, window by window, the events of the recoding that random magnitudes meet about twice in 40 000 at 16-bit
windows; the corpora below put at least one term into every (event, window, width) cell the model says can be reached:
hook_corpus for s2k_debug_msm_terms (any magnitude below 2^128), public_corpus for s2k_multi_scalar_mult (scalars
k = +-m1 +- m2 lambda mod n whose split gives back exactly the chosen halves)."""
import os
import random
import re

from pointset_model import A1, B1, B2, LAM, N, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSM_SRC = os.path.join(ROOT, "secp256k1_voi_amd", "csrc", "msm.hip")
SCALAR_BITS = 128
FINE = 256                     # keys per coarse bucket: the key range is padded to a multiple of it
TERM_NEG = 0x80000000
WIDTHS = (8, 12, 16)
# the events of a window below the top, and of the top window (v = digit + carry coming in, half = 2^(c-1), full = 2^c)
LOW_EVENTS = ("half", "half+1", "full", "one", "zero", "carry_in")
TOP_EVENTS = ("top_half", "top_half+1", "top_full-1", "top_full", "one", "zero", "carry_in")
# The largest halves the split can return.  k1 = f1 a1 + f2 a2 and k2 = -(f1 b1 + f2 b2) with the rounding remainders
# |f1|, |f2| <= 1/2 (a2 = a1 - b1, b2 = a1: the lattice basis of the split), so |k1| <= (a1 + a2) / 2 = 0xA2A8918C.. * 2^96 and
# |k2| <= (|b1| + b2) / 2 = 0x8A652879.. * 2^96, plus the few units the 384-bit approximations of the quotients can add.
# Random scalars stay a little below (both remainders have to be near 1/2 at once): 200 000 of them came to 0xA276.. and 0x8A3B...
GLV_BOUND_1 = (A1 + (A1 - B1)) // 2 + 4
GLV_BOUND_2 = (-B1 + B2) // 2 + 4


def thresholds():
    """(log2 of the term count from which msm_setup takes 16-bit windows, term count from which it takes 12-bit ones), read
    out of the source; a change of the expression fails here and asks for the model to be restated."""
    src = open(MSM_SRC).read()
    m = re.search(r"g\.c = force_c \? force_c : \(n >= \(\(size_t\)1 << c16_from_log2\) \? 16 : \(n >= (\d+) \? 12 : 8\)\);", src)
    d = re.search(r'getenv\("S2K_MSM_C16_FROM_LOG2"\);\s*return e \? atoi\(e\) : (\d+);', src)
    assert m and d, "msm_setup no longer chooses the window width as msm_digits_model.py restates it"
    assert "g.nw = (SCALAR_BITS + g.c - 1) / g.c;" in src and "g.nb = 1u << (g.c - 1);" in src and "g.nslot = g.nw + 1;" in src
    assert "m.nkeys = align_up((size_t)g.nslot * g.nb, FINE);" in src and "FINE_BITS = 8, FINE = 1u << FINE_BITS" in src
    return int(d.group(1)), int(m.group(1))


def core_constants():
    """the constants of the bucket pass and its stitching the device tests lean on, read out of the source: shortest range,
    ranges a bucket may span before it is queued, the queue's capacity, lanes that fill the chip once"""
    src = open(MSM_SRC).read()
    m = re.search(r"constexpr uint32_t STITCH_SERIAL = (\d+), STITCH_BIG_CAP = (\d+);", src)
    lmin = re.search(r"constexpr uint32_t MSM_L_MIN = (\d+);", src)
    lanes = re.search(r"constexpr uint32_t MSM_LANES = 256u \* 4u \* 64u \* S2K_MSM_WAVES;", src)
    waves = re.search(r"#define S2K_MSM_WAVES (\d+)", src)
    assert m and lmin and lanes and waves, "the constants of the bucket pass are no longer written as msm_digits_model.py reads them"
    # what the tests assume of the code around them: the queue test, and the length of a range
    assert "if (k_hi - k_lo > STITCH_SERIAL) {" in src and "if (pos < STITCH_BIG_CAP) {" in src
    assert "size_t la = (pairs_a + target_a - 1) / target_a" in src and "if (la < MSM_L_MIN) la = MSM_L_MIN;" in src
    return dict(STITCH_SERIAL=int(m.group(1)), STITCH_BIG_CAP=int(m.group(2)), L_MIN=int(lmin.group(1)),
                LANES=256 * 4 * 64 * int(waves.group(1)))


def geometry(nterms, force_c=0):
    """c, nw, nb, nslot, nkeys as msm_setup lays them out for nterms terms (force_c: the width the test hook forces)."""
    c16_log2, c12_from = thresholds()
    c = force_c or (16 if nterms >= 1 << c16_log2 else (12 if nterms >= c12_from else 8))
    nw = (SCALAR_BITS + c - 1) // c
    nb = 1 << (c - 1)
    nslot = nw + 1
    return dict(c=c, nw=nw, nb=nb, nslot=nslot, nkeys=(nslot * nb + FINE - 1) // FINE * FINE)


def nwindows(c):
    return (SCALAR_BITS + c - 1) // c


def top_bits(c):
    return SCALAR_BITS - c * (nwindows(c) - 1)


def digit(mag, w, c):
    """msm_digit: window w of a magnitude below 2^128 (the words above it are zero)"""
    return (mag >> (w * c)) & ((1 << c) - 1)


def walk(mag, c):
    """msm_for_digits window by window: (w, v, carry_in, negative, |digit|) for every window, entries and empty ones alike"""
    assert 0 <= mag < 1 << SCALAR_BITS
    nw, half, full = nwindows(c), 1 << (c - 1), 1 << c
    carry, out = 0, []
    for w in range(nw):
        v = digit(mag, w, c) + carry
        neg = w + 1 < nw and v > half
        out.append((w, v, carry, neg, full - v if neg else v))
        carry = 1 if neg else 0
    return out


def for_digits(mag, c):
    """[(key, negative)] : the calls msm_for_digits makes for a magnitude"""
    nb = 1 << (c - 1)
    return [(w * nb + m - 1, neg) for w, _, _, neg, m in walk(mag, c) if m]


def signed_digits(mag, c):
    return [-m if neg else m for _, _, _, neg, m in walk(mag, c)]


def classify(mag, c):
    """per window, the set of events the recoding of `mag` meets there"""
    nw, half, full = nwindows(c), 1 << (c - 1), 1 << c
    out = []
    for w, v, cin, neg, m in walk(mag, c):
        ev = set()
        top = w == nw - 1
        if cin:
            ev.add("carry_in")
        if m == 0 and v == 0:
            ev.add("zero")
        if m == 1:
            ev.add("one")
        if top:
            for name, val in (("top_half", half), ("top_half+1", half + 1), ("top_full-1", full - 1), ("top_full", full)):
                if v == val:
                    ev.add(name)
        else:
            for name, val in (("half", half), ("half+1", half + 1), ("full", full)):
                if v == val:
                    ev.add(name)
        out.append(ev)
    return out


def reachable_cells(c, top_max=None):
    """the (event, window) cells a magnitude can reach at width c.  Window 0 has no carry coming in (so no `full` either);
    a top window of fewer than c bits (c = 12: 8 bits) never reaches half.  top_max: the largest top-window value v the
    magnitudes can have (default: any magnitude below 2^128)."""
    nw, half, full = nwindows(c), 1 << (c - 1), 1 << c
    cells = set()
    for w in range(nw - 1):
        for ev in LOW_EVENTS:
            if w == 0 and ev in ("full", "carry_in"):
                continue
            cells.add((ev, w))
    vmax = (1 << top_bits(c)) if top_max is None else top_max          # all ones plus a carry
    for ev, val in (("top_half", half), ("top_half+1", half + 1), ("top_full-1", full - 1), ("top_full", full), ("one", 1), ("zero", 0)):
        if val <= vmax:
            cells.add((ev, nw - 1))
    cells.add(("carry_in", nw - 1))
    return cells


def cells_of(mags, c):
    got = set()
    for mag in mags:
        for w, evs in enumerate(classify(mag, c)):
            got.update((ev, w) for ev in evs)
    return got


def words(c):
    """the six words of the patterns: 0x8000, 0x8001, 0x7FFF, 0xFFFF, 0, 1 at c = 16"""
    half, full = 1 << (c - 1), 1 << c
    return [half, half + 1, half - 1, full - 1, 0, 1]


def pattern(word, c, length=None):
    """`word` in each of the lowest `length` windows (default: all of them), cut to 128 bits"""
    nw = nwindows(c)
    return sum(word << (c * w) for w in range(nw if length is None else length)) & ((1 << SCALAR_BITS) - 1)


def targeted(c, below_top_only=False):
    """magnitudes built for one cell each: (event, window) -> magnitude"""
    nw, half, full = nwindows(c), 1 << (c - 1), 1 << c
    t = {}
    for w in range(nw - 1):
        sh = c * w
        t[("half", w)] = half << sh
        t[("half+1", w)] = (half + 1) << sh
        t[("one", w)] = 1 << sh
        t[("zero", w)] = (3 << (sh + c)) | (2 if w else 0)        # digits around it, none in it
        if w:
            carry = (half + 1) << (sh - c)                        # the window below: negative, carries one into w
            t[("full", w)] = ((full - 1) << sh) | carry
            t[("carry_in", w)] = (5 << sh) | carry
            t[("half by carry", w)] = ((half - 1) << sh) | carry
            t[("half+1 by carry", w)] = (half << sh) | carry
            t[("one by carry", w)] = ((full - 2) << sh) | carry    # v = 2^c - 1: digit -1
    if below_top_only:
        return t
    sh, carry = c * (nw - 1), (half + 1) << (c * (nw - 2))
    tb = top_bits(c)
    t[("one", nw - 1)] = 1 << sh
    t[("zero", nw - 1)] = 7
    t[("carry_in", nw - 1)] = (2 << sh) | carry
    if tb == c:
        t[("top_half", nw - 1)] = half << sh
        t[("top_half+1", nw - 1)] = (half + 1) << sh
        t[("top_full-1", nw - 1)] = (full - 1) << sh
        t[("top_full", nw - 1)] = ((full - 1) << sh) | carry
        t[("top_half by carry", nw - 1)] = ((half - 1) << sh) | carry
    else:
        t[("top all ones", nw - 1)] = ((1 << tb) - 1) << sh
        t[("top all ones and a carry", nw - 1)] = (((1 << tb) - 1) << sh) | carry
    return t


def smallest_with_full_top(c):
    """the smallest magnitude whose top-window digit is 2^c (the last key of the key range): all ones on top, `half` in every
    window below it and half + 1 in window 0, so that a carry ripples through every window"""
    assert top_bits(c) == c
    nw, half, full = nwindows(c), 1 << (c - 1), 1 << c
    return ((full - 1) << (c * (nw - 1))) | pattern(half, c, nw - 1) | 1


def named_magnitudes(c):
    """the full-range magnitudes every hook corpus carries, by name"""
    nw = nwindows(c)
    out = {"2^128 - 1": (1 << 128) - 1, "2^128 - 2^(c (nw - 1) - 1)": (1 << 128) - (1 << (c * (nw - 1) - 1)),
           "2^128 - 2^(c (nw - 1) - 1) + 1": (1 << 128) - (1 << (c * (nw - 1) - 1)) + 1, "0": 0, "1": 1, "2^127": 1 << 127}
    if top_bits(c) == c:
        out["smallest with top digit 2^c"] = smallest_with_full_top(c)
    for w in words(c):
        out["0x%x per window" % w] = pattern(w, c)
    return out


def hook_corpus(c, count=None, seed=5):
    """[(name, magnitude)]: the named magnitudes, one per reachable cell, then random ones up to `count` terms"""
    out = list(named_magnitudes(c).items())
    out += [("%s at window %d" % k, v) for k, v in sorted(targeted(c).items(), key=lambda kv: (kv[0][1], kv[0][0]))]
    rnd = random.Random(seed * 100 + c)
    if count is not None:
        assert len(out) <= count, (len(out), count)
        out += [("random", rnd.getrandbits(128)) for _ in range(count - len(out))]
    return out


# ---- one point in one chosen bucket of the 16-bit reduction (k_msm_fold .. k_msm_final16) -------------------------------
# key (h, l) of window w has the magnitude 256 h + l + 1; the rows 128 .. 255 are the top window's second slot
FOLD_H_LOW, FOLD_H_TOP = [0, 1, 2, 4, 8, 16, 32, 64, 127], [128, 255]
FOLD_L = [0, 1, 3, 7, 15, 31, 63, 127, 254, 255]


def fold_probes():
    """[(w, h, l, magnitude)]: digit m = 256 h + l + 1 in window w and nothing else - except m = 2^16, which no magnitude has as
    a digit of its own: it is 0xFFFF plus a carry out of the window below (which then holds -0x7FFF)"""
    out = []
    for w in range(8):
        for h in FOLD_H_LOW + (FOLD_H_TOP if w == 7 else []):
            for l in FOLD_L:
                m = 256 * h + l + 1
                out.append((w, h, l, m << (16 * w) if m < 1 << 16 else (0xFFFF << 112) | (0x8001 << 96)))
    return out


# ---- the public path: scalars whose endomorphism split gives chosen halves -------------------------------------------
def scalar_of(m1, neg1, m2, neg2):
    return ((-m1 if neg1 else m1) + (-m2 if neg2 else m2) * LAM) % N


def round_trips(m1, neg1, m2, neg2):
    a1, s1, a2, s2 = split(scalar_of(m1, neg1, m2, neg2))
    return a1 == m1 and a2 == m2 and (m1 == 0 or s1 == neg1) and (m2 == 0 or s2 == neg2)


def pattern_lengths(c):
    """windows a patterned half fills: the top window stays empty, so every such half is below 2^127.  (A half that fills all
    windows need not come back from the split even below 2^127: (m1, m2) has to lie in the split's parallelogram, not in its
    bounding box - 0x7FFF.. in all eight windows as m2 beside m1 = 0 does not.)"""
    nw = nwindows(c)
    return [1, nw // 2, nw - 2, nw - 1]


def large_halves(c):
    """halves with a top-window digit, up to the split's bound and beyond it: the split returns some of them"""
    nw, half = nwindows(c), 1 << (c - 1)
    sh = c * (nw - 1)
    top = [1, 2, (1 << top_bits(c)) // 4, 0x51 << (top_bits(c) - 8), 0x8A << (top_bits(c) - 8), 0xA2 << (top_bits(c) - 8), (1 << top_bits(c)) - 1]
    out = [t << sh for t in top] + [(t << sh) | pattern(half + 1, c, nw - 1) for t in top]
    if top_bits(c) == c:
        out += [half << sh, (half + 1) << sh, pattern(half, c), pattern(half + 1, c)]
    return out


def public_candidates(c):
    """[(m1, neg1, m2, neg2)]: first the halves that vanish and one pattern pair (a call of three inputs holds them), then two
    targeted halves per scalar (every cell below the top window), then six words x six words x four sign pairs x four
    lengths of patterned halves"""
    half = 1 << (c - 1)
    cand = [(0, False, pattern(half + 1, c, nwindows(c) - 1), True), (pattern(half, c, nwindows(c) - 1), True, 0, False),
            (pattern(half + 1, c, nwindows(c) - 1), False, pattern((1 << c) - 1, c, nwindows(c) - 1), True)]
    t = [v for _, v in sorted(targeted(c, below_top_only=True).items(), key=lambda kv: (kv[0][1], kv[0][0]))]
    t += [t[0]] * (len(t) & 1)
    for i in range(0, len(t), 2):
        cand.append((t[i], bool(i & 2), t[i + 1], not (i & 4)))
    signs = [(False, False), (False, True), (True, False), (True, True)]
    for ln in pattern_lengths(c):
        for w1 in words(c):
            for w2 in words(c):
                for s1, s2 in signs:
                    cand.append((pattern(w1, c, ln), s1, pattern(w2, c, ln), s2))
    for big in large_halves(c):
        for s1, s2 in signs:
            cand += [(big, s1, 1, s2), (3, s1, big, s2)]
    return cand


def public_corpus(c):
    """(kept, dropped): kept = [(k, m1, neg1, m2, neg2)] whose model split returns exactly the halves chosen; dropped = the
    candidates that do not (only halves of 2^127 and more may: the corpus test asserts it)"""
    kept, dropped, seen = [], [], set()
    for m1, s1, m2, s2 in public_candidates(c):
        if round_trips(m1, s1, m2, s2):
            k = scalar_of(m1, s1, m2, s2)
            if k not in seen:
                seen.add(k)
                kept.append((k, m1, s1, m2, s2))
        else:
            dropped.append((m1, s1, m2, s2))
    return kept, dropped
