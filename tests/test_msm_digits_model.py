"""The model of the bucket method's signed recoding (msm_digits_model.py) against plain arithmetic, and the corpora the device
tests run (test_gpu_msm_terms.py) against the model: every (event, window, width) cell the model says can be reached holds a
term.  No device."""
import random

import pytest

import msm_digits_model as M
from pointset_model import N, split


def boundary_pool(c):
    pool = [v for _, v in M.hook_corpus(c)]
    for v in list(pool):
        pool += [(v + 1) & ((1 << 128) - 1), (v - 1) & ((1 << 128) - 1)]
    return pool


@pytest.mark.parametrize("c", M.WIDTHS)
def test_digits_sum_to_the_magnitude(c):
    rnd = random.Random(c)
    nw, nb = M.nwindows(c), 1 << (c - 1)
    nkeys = M.geometry(1, c)["nkeys"]
    for mag in boundary_pool(c) + [rnd.getrandbits(128) for _ in range(20000)] + [rnd.getrandbits(rnd.randrange(1, 129)) for _ in range(2000)]:
        d = M.signed_digits(mag, c)
        assert len(d) == nw and sum(x << (c * w) for w, x in enumerate(d)) == mag
        assert all(abs(x) <= nb for x in d[:-1]) and 0 <= d[-1] <= 2 * nb
        keys = M.for_digits(mag, c)
        assert len(keys) == sum(1 for x in d if x)
        for key, neg in keys:
            assert 0 <= key < (nw + 1) * nb <= nkeys             # keys stay below nslot * nb
            w = min(key // nb, nw - 1)
            m = key - w * nb + 1
            assert d[w] == (-m if neg else m)
            assert not (neg and w == nw - 1)                      # the top window is unsigned


def test_top_window_of_12_bit_windows_stays_in_its_first_slot():
    c, rnd = 12, random.Random(12)
    nw, nb = M.nwindows(c), 1 << 11
    assert M.top_bits(c) == 8
    for mag in boundary_pool(c) + [rnd.getrandbits(128) for _ in range(20000)]:
        top = M.signed_digits(mag, c)[-1]
        assert 0 <= top <= 256
        assert all(key < nw * nb for key, _ in M.for_digits(mag, c))


def test_geometry_follows_the_source():
    c16, c12 = M.thresholds()
    assert (c16, c12) == (13, 256)
    for n, c in ((1, 8), (c12 - 1, 8), (c12, 12), ((1 << c16) - 1, 12), (1 << c16, 16), (1 << 20, 16)):
        g = M.geometry(n)
        assert g["c"] == c and g["nw"] * c >= 128 > (g["nw"] - 1) * c
    # the constants the device tests read: the queue-overflow case (8 x 525 buckets of 124 entries and more, ranges of L_MIN
    # entries at 65536 terms) still overflows the queue and still makes every bucket oversized
    k = M.core_constants()
    assert 8 * 525 > k["STITCH_BIG_CAP"] and 124 > (k["STITCH_SERIAL"] + 1) * k["L_MIN"] and 65536 * 8 <= k["L_MIN"] * k["LANES"]
    assert M.geometry(5, 16) == dict(c=16, nw=8, nb=32768, nslot=9, nkeys=9 * 32768)
    assert M.geometry(5, 12) == dict(c=12, nw=11, nb=2048, nslot=12, nkeys=12 * 2048)
    assert M.geometry(5, 8) == dict(c=8, nw=16, nb=128, nslot=17, nkeys=2304)          # 17 x 128 = 2176, padded to 9 x 256


@pytest.mark.parametrize("c", M.WIDTHS)
def test_hook_corpus_fills_every_reachable_cell(c):
    corpus = M.hook_corpus(c)
    assert len(corpus) <= 255                                     # fits a call that takes 8-bit windows by itself
    need, got = M.reachable_cells(c), M.cells_of([v for _, v in corpus], c)
    assert need <= got, sorted(need - got)
    assert got <= need, sorted(got - need)                        # and the model's "unreachable" is not reached
    # each targeted magnitude meets its own cell
    for (ev, w), v in M.targeted(c).items():
        if ev in M.LOW_EVENTS + M.TOP_EVENTS:
            assert ev in M.classify(v, c)[w], (ev, w, hex(v))
    named = M.named_magnitudes(c)
    nw, nb = M.nwindows(c), 1 << (c - 1)
    last_key = (nw + 1) * nb - 1
    if M.top_bits(c) == c:
        # the last key of the key range: digit 2^c in the top window.  2^128 - 1 reaches it by a carry through every window; the
        # smallest magnitude that does is NOT 2^128 - 2^(c (nw - 1) - 1): its window below the top is exactly half, which stays
        # positive (top digit 2^c - 1), one more does not carry either; the smallest has half in every window and half + 1 in the lowest
        assert M.for_digits(named["2^128 - 1"], c) == [(0, True), (last_key, False)]
        assert M.for_digits(named["2^128 - 2^(c (nw - 1) - 1)"], c) == [((nw - 1) * nb - 1, False), (last_key - 1, False)]
        small = named["smallest with top digit 2^c"]
        assert M.for_digits(small, c)[-1] == (last_key, False) and M.for_digits(small - 1, c)[-1] == (last_key - 1, False)
    else:
        assert max(k for v in named.values() for k, _ in M.for_digits(v, c)) < nw * nb


@pytest.mark.parametrize("c", M.WIDTHS)
def test_public_corpus_round_trips_and_fills_the_cells_below_the_top(c):
    kept, dropped = M.public_corpus(c)
    nw = M.nwindows(c)
    for k, m1, s1, m2, s2 in kept:
        a1, n1, a2, n2 = split(k)
        assert (a1, a2) == (m1, m2) and (m1 == 0 or n1 == s1) and (m2 == 0 or n2 == s2)
        assert 0 <= k < N
    # patterned halves below 2^127 round-trip without exception; larger ones may be dropped
    small = [d for d in dropped if d[0] < 1 << 127 and d[2] < 1 << 127]
    assert not small, [(hex(a), s, hex(b), t) for a, s, b, t in small]
    halves = [m for _, m1, _, m2, _ in kept for m in (m1, m2)]
    need = {cell for cell in M.reachable_cells(c) if cell[1] < nw - 1}
    got = M.cells_of(halves, c)
    assert need <= got, sorted(need - got)
    assert any(m1 == 0 for _, m1, _, _, _ in kept[:3]) and any(m2 == 0 for _, _, _, m2, _ in kept[:3])
    top = max(M.signed_digits(m, c)[-1] for m in halves)
    print("c = %d: %d scalars kept, %d candidates of 2^127 and more dropped; top-window cells reached: %s; largest top digit %d of %d"
          % (c, len(kept), len(dropped), sorted(ev for ev, w in got if w == nw - 1), top, 1 << M.top_bits(c)))
    # what a call of the smallest width holds: the cells of 8-bit windows fit 127 inputs
    if c == 8:
        first = [m for _, m1, _, m2, _ in kept[:127] for m in (m1, m2)]
        assert need <= M.cells_of(first, c)


def test_split_halves_stay_inside_the_bound():
    """what the split keeps out of the public path's key range: the top digit of a half stays below 0xA2A9 of 0x10000 at
    16-bit windows (0xA3 of 0x100 at 8-bit ones), so the upper part of the extra slot is reached by raw 128-bit terms only"""
    rnd = random.Random(7)
    m1 = m2 = 0
    ks = [rnd.randrange(N) for _ in range(20000)] + [N - 1, N // 2, N // 2 + 1, 1, 0]
    for c in M.WIDTHS:
        ks += [k for k, *_ in M.public_corpus(c)[0]]
    for k in ks:
        a1, _, a2, _ = split(k)
        m1, m2 = max(m1, a1), max(m2, a2)
    assert m1 <= M.GLV_BOUND_1 and m2 <= M.GLV_BOUND_2
    assert M.GLV_BOUND_1 >> 112 == 0xA2A8 and M.GLV_BOUND_2 >> 112 == 0x8A65
    assert m1 >> 120 >= 0x9F and m2 >> 120 >= 0x87               # the samples come close: the bound is not loose


def test_fold_probes_cover_every_bit_plane():
    """the single-bucket probes of the 16-bit reduction: each sits in the key it names, and every bit plane of each of the 17
    weighted sums (8 sums of row sums with weights h, 9 sums of column sums with weights l + 1) carries a probe alone - a
    weight with that single bit set"""
    pr = M.fold_probes()
    for w, h, l, mag in pr:
        keys = M.for_digits(mag, 16)
        assert (w * 32768 + 256 * h + l, False) in keys and len(keys) == (1 if 256 * h + l + 1 < 65536 else 2)
    for ws in range(8):
        for b in range(8 if ws == 7 else 7):
            assert any(w == ws and h == 1 << b for w, h, l, _ in pr)
    for slot in range(9):
        for b in range(9):
            assert any((w if h < 128 else 8) == slot and l + 1 == 1 << b for w, h, l, _ in pr)
