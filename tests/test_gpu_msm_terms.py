"""The bucket method of msm.hip on chosen 128-bit terms (s2k_debug_msm_terms: the product's sort, bucket pass, reduction and
tail behind a fill kernel of the hook) and on scalars whose endomorphism split gives chosen halves (s2k_multi_scalar_mult).
Expected points are big integers on known discrete logarithms - P_i = d_i G, result = (sum +-m_i d_i mod n) G - taken from the
CPU oracle, never from the engine; the sort's offset[] / list[] are compared with msm_digits_model.py as a multiset per key (the
order inside a bucket comes from atomics).  Everything is exact: equal bytes, equal multisets."""
import random

import numpy as np
import pytest

import msm_digits_model as M
from pointset_model import N
from pyref import b32

pytestmark = pytest.mark.gpu
IDENT = bytes(65)
ERR_ARG = -3
POOL = 8192
K = M.core_constants()                  # STITCH_SERIAL, STITCH_BIG_CAP, L_MIN, LANES as msm.hip has them
STITCH_SERIAL, STITCH_BIG_CAP, L_MIN = K["STITCH_SERIAL"], K["STITCH_BIG_CAP"], K["L_MIN"]


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(oracle):
    """8192 points of known discrete logarithm, as an (n, 65) array"""
    rnd = random.Random(4242)
    d = [rnd.randrange(1, N) for _ in range(POOL)]
    pts = np.frombuffer(b"".join(oracle.scalar_base_mult_vartime(b32(x)) for x in d), np.uint8).reshape(POOL, 65).copy()
    return d, pts


def b16(v):
    return int(v).to_bytes(16, "big")


def mags_array(mags):
    return np.frombuffer(b"".join(b16(m) for m in mags), np.uint8).reshape(len(mags), 16)


def point_of(oracle, k):
    k %= N
    return IDENT if k == 0 else oracle.scalar_base_mult_vartime(b32(k))


def expected(oracle, mags, dlogs, signs=None, present=None):
    tot = 0
    for i, (m, d) in enumerate(zip(mags, dlogs)):
        if present is not None and not present[i]:
            continue
        tot += -m * d if signs is not None and signs[i] else m * d
    return point_of(oracle, tot)


def model_entries(mags, present, c):
    keys, ents = [], []
    for i, m in enumerate(mags):
        if present is not None and not present[i]:
            continue
        for key, neg in M.for_digits(m, c):
            keys.append(key)
            ents.append(i | (M.TERM_NEG if neg else 0))
    return np.asarray(keys, dtype=np.int64), np.asarray(ents, dtype=np.uint32)


def check_dump(res, mags, present, c):
    """offset[] is the exclusive scan of the model's count per key, and every key holds the model's entries in some order"""
    nkeys = res["nkeys"]
    keys, ents = model_entries(mags, present, c)
    counts = np.bincount(keys, minlength=nkeys) if keys.size else np.zeros(nkeys, dtype=np.int64)
    assert counts.size == nkeys                                     # no model key beyond the key range
    off = res["offset"].astype(np.int64)
    assert off.size == nkeys + 1 and off[0] == 0
    assert np.array_equal(np.diff(off), counts)
    assert res["list_len"] == keys.size == res["list"].size
    dev_keys = np.repeat(np.arange(nkeys), counts)
    a, b = np.lexsort((res["list"], dev_keys)), np.lexsort((ents, keys))
    assert np.array_equal(res["list"][a], ents[b])
    return counts


def check_geometry(res, nterms, force_c):
    g = M.geometry(nterms, force_c)
    assert {k: res[k] for k in g} == g
    # msm_core's own cut, as the call ran it (one-part flow, no tuning variable set), against the constants read out of msm.hip:
    # the tests use L_A to know where range borders fall; the sums and the sort's arrays check the rest of the core
    assert res["fold16"] == (1 if g["c"] == 16 else 0)
    assert res["L_A"] == max(L_MIN, -(-nterms * g["nw"] // K["LANES"]))
    assert res["nlanes"] == -(-nterms * g["nw"] // res["L_A"])


def run(eng, oracle, pool, mags, idx, signs=None, present=None, force_c=0, dump=True):
    """one call of the hook on the terms mags[i] * (+-pool point idx[i]) (present[i] false: an all-zero record), checked against
    the dlogs and, with dump, against the model's keys"""
    d, pts = pool
    p = pts[np.asarray(idx)].copy()
    if present is not None:
        p[~np.asarray(present, dtype=bool)] = 0
    res = eng.debug_msm_terms(mags_array(mags), p, None if signs is None else np.asarray(signs, dtype=np.uint8), window_bits=force_c, dump=dump)
    check_geometry(res, len(mags), force_c)
    want = expected(oracle, mags, [d[i] for i in idx], signs, present)
    assert res["out"] == want, "the sum differs from the big-integer result"
    if dump:
        res["counts"] = check_dump(res, mags, present, res["c"])
    return res


# ---- the digit corpus ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nterms,force_c,c", [(None, 0, 8), (255, 0, 8), (256, 0, 12), (300, 16, 16), (8192, 0, 16), (300, 8, 8), (120, 12, 12),
                                                (100, 16, 16)])
def test_digit_corpus(eng, oracle, pool, nterms, force_c, c):
    corpus = M.hook_corpus(c, nterms)
    mags = [v for _, v in corpus]
    n = len(mags)
    rnd = random.Random(n * 31 + c)
    idx = list(range(n))
    signs = [rnd.randrange(2) for _ in range(n)]
    res = run(eng, oracle, pool, mags, idx, signs, None, force_c)
    assert res["c"] == c
    nb, nw = res["nb"], res["nw"]
    counts = res["counts"]
    if M.top_bits(c) == c:
        assert counts[(nw + 1) * nb - 1] >= 2                       # the last key of the range: 2^128 - 1 and the smallest such magnitude
        assert counts[nw * nb:(nw + 1) * nb].sum() >= 4            # the extra slot of the top window
    else:
        assert counts[nw * nb:].sum() == 0
    # the same terms with some of them identity records (flag 0: skipped, whatever their magnitude)
    present = [rnd.random() < 0.8 for _ in range(n)]
    run(eng, oracle, pool, mags, idx, signs, present, force_c)


# ---- one point in one chosen bucket of the 16-bit reduction --------------------------------------------------------------
probes = M.fold_probes


def test_single_bucket_probes(eng, oracle, pool):
    d, pts = pool
    for i, (w, h, l, mag) in enumerate(probes()):
        res = eng.debug_msm_terms(mags_array([mag]), pts[i:i + 1], window_bits=16)
        assert res["fold16"] == 1 and res["c"] == 16
        assert res["out"] == point_of(oracle, mag * d[i]), "probe w = %d, h = %d, l = %d" % (w, h, l)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_many_probes_together(eng, oracle, pool, seed):
    pr = probes()
    rnd = random.Random(seed)
    if seed:
        pr = rnd.sample(pr, [0, 17, 200, 500][seed])
    mags = [p[3] for p in pr]
    run(eng, oracle, pool, mags, list(range(len(mags))), [rnd.randrange(2) for _ in mags], None, 16)


# ---- empty and cancelling slots ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("force_c,c", [(0, 8), (12, 12), (16, 16)])
def test_empty_window(eng, oracle, pool, force_c, c):
    nw, rnd = M.nwindows(c), random.Random(c)
    for w in (0, 1, nw // 2, nw - 2, nw - 1):
        mags = []
        for _ in range(40):
            m = rnd.getrandbits(128) & ~(((1 << c) - 1) << (c * w))
            if w:                                                   # nothing carried in either: the window below stays positive
                m &= ~(1 << (c * w - 1))
            mags.append(m)
        res = run(eng, oracle, pool, mags, list(range(40)), None, None, force_c)
        nb = res["nb"]
        assert res["counts"][w * nb:(w + 1) * nb].sum() == 0 and (w < nw - 1 or res["counts"][nw * nb:].sum() == 0)


@pytest.mark.parametrize("force_c,c", [(0, 8), (12, 12), (16, 16)])
def test_slot_that_sums_to_the_identity(eng, oracle, pool, force_c, c):
    """P in bucket 2 and -2P in bucket 1 of one window: neither bucket is the identity, their weighted sum is"""
    d, pts = pool
    nw = M.nwindows(c)
    p2 = np.frombuffer(oracle.point_double(pts[0].tobytes()), np.uint8)
    for w in (0, nw // 2, nw - 1):
        others = [(3 << (c * v)) for v in range(nw) if v != w]
        mags = [2 << (c * w), 1 << (c * w)] + others
        p = np.concatenate([pts[0:1], p2[None, :], pts[1:1 + len(others)]])
        signs = np.asarray([0, 1] + [0] * len(others), dtype=np.uint8)
        for with_others in (True, False):
            k = len(mags) if with_others else 2
            res = eng.debug_msm_terms(mags_array(mags[:k]), p[:k], signs[:k], window_bits=force_c, dump=True)
            assert res["c"] == c
            want = point_of(oracle, sum(m * x for m, x in zip(others, d[1:])) if with_others else 0)
            assert res["out"] == want
            off = res["offset"]
            assert off[w * res["nb"] + 1] - off[w * res["nb"]] == 1 and off[w * res["nb"] + 2] - off[w * res["nb"] + 1] == 1


@pytest.mark.parametrize("force_c", [0, 12, 16])
def test_no_term_at_all(eng, oracle, pool, force_c):
    d, pts = pool
    rnd = random.Random(3)
    mags = [rnd.getrandbits(128) for _ in range(50)]
    res = eng.debug_msm_terms(mags_array(mags), np.zeros((50, 65), np.uint8), window_bits=force_c, dump=True)       # all flag 0
    assert res["out"] == IDENT and res["list_len"] == 0 and not res["offset"].any()
    res = eng.debug_msm_terms(mags_array([0] * 50), pts[:50], window_bits=force_c, dump=True)                        # all magnitudes 0
    assert res["out"] == IDENT and res["list_len"] == 0 and not res["offset"].any()


# ---- a bucket whose incomplete additions meet ZZ = 0 late ----------------------------------------------------------------
@pytest.mark.parametrize("force_c", [0, 16])
@pytest.mark.parametrize("j", range(2, 10))
def test_late_exceptional_addition(eng, oracle, pool, j, force_c):
    """one bucket holding P1 .. Pj and -(P1 + .. + Pj): in any order the last addition of the walk is X + (-X).  Ranges are 8
    entries long: the sets of 9 and more cross a range border, and a few terms in a lower bucket shift where it falls."""
    d, pts = pool
    c = force_c or 8
    base = 100 * j
    ds = d[base:base + j]
    x = np.frombuffer(point_of(oracle, sum(ds)), np.uint8)
    q = pts[base + 20:base + 21]
    for w, m in ((0, 5), (M.nwindows(c) - 1, 77)):
        mag = m << (c * w)
        for shift in (0, 3):
            lead_p, lead_m = pts[base + 30:base + 30 + shift], [1 << (c * w)] * shift        # `shift` terms in the slot's first bucket
            lead = sum(d[base + 30:base + 30 + shift]) << (c * w)
            p = np.concatenate([lead_p, pts[base:base + j], x[None, :]])
            signs = np.asarray([0] * (shift + j) + [1], dtype=np.uint8)
            res = eng.debug_msm_terms(mags_array(lead_m + [mag] * (j + 1)), p, signs, window_bits=force_c, dump=True)
            assert res["L_A"] == L_MIN and res["c"] == c
            key = w * res["nb"] + m - 1
            assert res["offset"][key + 1] - res["offset"][key] == j + 1
            assert res["out"] == point_of(oracle, lead), "the set alone (j = %d, window %d, shift %d)" % (j, w, shift)
            # ... and with one more point in the bucket
            res = eng.debug_msm_terms(mags_array(lead_m + [mag] * (j + 2)), np.concatenate([p, q]), np.append(signs, 0).astype(np.uint8),
                                      window_bits=force_c)
            assert res["out"] == point_of(oracle, lead + mag * d[base + 20]), "the set and Q (j = %d, window %d, shift %d)" % (j, w, shift)


# ---- more oversized buckets than the stitch queue holds ------------------------------------------------------------------
def test_stitch_queue_overflow(eng, oracle, pool):
    """65536 terms at 16-bit windows, every digit one of 525 values <= 2^15: 8 x 525 = 4200 buckets of 124 or 125 entries, ranges
    of 8 entries, so every bucket spans more than 8 ranges and 4200 > 4096 of them ask for the queue (the 8, 8 and 4096 are
    read out of msm.hip: a larger queue fails the last assertion instead of passing without an overflow)"""
    d, pts = pool
    n, nv = 65536, 525
    rnd = random.Random(525)
    vals = [1, 1 << 15] + rnd.sample(range(2, 1 << 15), nv - 2)
    mult = [1, 2, 4, 8, 11, 13, 16, 17]                             # coprime to 525: every value takes 124 or 125 terms per window,
    mags = [sum(vals[(i * mult[w] + 37 * w) % nv] << (16 * w) for w in range(8)) for i in range(n)]
    idx = [i % POOL for i in range(n)]                              # ... and the 8 copies of a point never share a bucket
    res = run(eng, oracle, pool, mags, idx, None, None, 0)
    assert res["c"] == 16 and res["L_A"] == L_MIN
    sizes = res["counts"][res["counts"] > 0]
    assert sizes.size == 8 * nv and sizes.min() == 124 and sizes.max() == 125
    assert sizes.min() > (STITCH_SERIAL + 1) * res["L_A"]           # more than STITCH_SERIAL range borders inside every bucket
    assert res["big"] == 8 * nv > STITCH_BIG_CAP


# ---- the public call: parse, split, then the same core -------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 127, 200, 300, 4096, 5000])
def test_multi_scalar_mult_on_patterned_halves(eng, oracle, pool, n):
    d, pts = pool
    c = M.geometry(2 * n)["c"]
    kept, _ = M.public_corpus(c)
    rnd = random.Random(n)
    base = [k for k, *_ in kept]                                    # the corpus first; beyond it, its scalars again (on other points) and random ones
    ks = [base[i % len(base)] if i < len(base) or i % 2 else rnd.randrange(N) for i in range(n)]
    if n >= 127:
        halves = [m for k, m1, _, m2, _ in kept[:n - 1] for m in (m1, m2)]      # (the last input is the identity record below)
        assert {cell for cell in M.reachable_cells(c) if cell[1] < M.nwindows(c) - 1} <= M.cells_of(halves, c)
    p = pts[:n].copy()
    skip = n - 1 if n > 3 else n                                    # one identity input (a call of three keeps its three scalars)
    if skip < n:
        p[skip] = 0
    scalars = np.frombuffer(b"".join(b32(k) for k in ks), np.uint8).reshape(n, 32)
    got = eng.multi_scalar_mult(scalars, p)
    want = point_of(oracle, sum(k * x for i, (k, x) in enumerate(zip(ks, d)) if i != skip))
    assert got == want
    if n <= 300:
        assert got == oracle.multi_scalar_mult_vartime([b32(k) for k in ks], [bytes(r) for r in p])


# ---- what the hook refuses -----------------------------------------------------------------------------------------------
def test_hook_refusals_then_a_good_call(eng, oracle, pool):
    import secp256k1_voi_amd as S
    d, pts = pool
    lib, h = eng._lib, eng._h
    mags, out, geom = mags_array([5, 6]), np.zeros(65, np.uint8), np.zeros(10, np.uint32)
    p = pts[:2].copy()
    offs, lst = np.zeros(9 * 32768 + 1, np.uint32), np.zeros(64, np.uint32)

    def call(nterms=2, points=p, wb=0, o=None, ocap=0, l=None, lcap=0, m=mags):
        return lib.s2k_debug_msm_terms(h, nterms, m.ctypes.data, points.ctypes.data, None, wb, out.ctypes.data, geom.ctypes.data,
                                       None if o is None else o.ctypes.data, ocap, None if l is None else l.ctypes.data, lcap)

    for wb in (-1, 1, 4, 7, 9, 15, 17, 24, 32):
        assert call(wb=wb) == ERR_ARG
    assert call(nterms=0) == ERR_ARG
    assert call(nterms=(1 << 22) + 1) == ERR_ARG                    # (refused before a byte of the buffers is read)
    assert call(nterms=1 << 40) == ERR_ARG
    assert call(o=offs, ocap=offs.size) == ERR_ARG                  # offsets without a list
    assert call(o=offs, ocap=100, l=lst, lcap=lst.size) == ERR_ARG  # offsets too short for the key range
    assert call(o=offs, ocap=offs.size, l=lst, lcap=1) == ERR_ARG   # list too short: 5 and 6 make one entry each
    bad = p.copy()
    bad[1, 64] ^= 1                                                 # not on the curve
    assert call(points=bad) == ERR_ARG
    bad = p.copy()
    bad[1, 0] = 2                                                   # not a record
    assert call(points=bad) == ERR_ARG
    bad = np.zeros((2, 65), np.uint8)
    bad[0, 40] = 1                                                  # neither a point nor all zero
    assert call(points=bad) == ERR_ARG
    assert lib.s2k_debug_msm_terms(None, 2, mags.ctypes.data, p.ctypes.data, None, 0, out.ctypes.data, geom.ctypes.data, None, 0, None, 0) == ERR_ARG
    with pytest.raises(S.EngineError):
        eng.debug_msm_terms(mags, p, window_bits=10)
    # the context is as good as before
    assert call(o=offs, ocap=offs.size, l=lst, lcap=lst.size) == 0
    assert out.tobytes() == point_of(oracle, 5 * d[0] + 6 * d[1]) and list(geom[:5]) == [8, 16, 128, 17, 2304] and geom[9] == 2
    run(eng, oracle, pool, [v for _, v in M.hook_corpus(8)], list(range(len(M.hook_corpus(8)))))
