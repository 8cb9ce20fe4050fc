"""The host-side plan of s2k_multi_scalar_mult_segments as a pure function (s2k_debug_msm_segments_plan, no device): which
terms go into which piece of the Straus path, which segments take the bucket method, and how much workspace the call
reserves - for random and adversarial offset arrays.  Plus the argument checks of the two entry points that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -3
LONG = 0x80000000
MAX_TERMS = 0x1FFFFFFF            # the limit s2k_multi_scalar_mult_device enforces


@pytest.fixture(scope="module")
def S():
    import secp256k1_voi_amd as S
    if not os.path.exists(S.LIB_PATH):
        S.build()
    S.load_library()
    return S


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def align(x, a):
    return (x + a - 1) // a * a


def workspace_bytes(n, n_seg, pieces, short_terms):
    """The carve of msm_seg.hip restated: status word, segment and piece descriptors, 33 digit bytes per half scalar and
    eight 64-byte table entries per term of the Straus path (indexed by the term's position among those), and
    one 27-word point per piece (planes of a stride rounded up to a wave); every block aligned to 256 bytes."""
    span = short_terms
    blocks = [256, n_seg * 8, pieces * 12, span * 2 * 33, span * 8 * 64, align(pieces, 64) * 27 * 4]
    return sum(align(b, 256) for b in blocks)


def check_plan(S, lens, T, X):
    lens = np.asarray(lens, dtype=np.int64)
    n, n_seg = int(lens.sum()), len(lens)
    off = offsets_of(lens)
    plan = S.msm_segments_plan(n, off, piece_terms=T, crossover=X)
    assert plan["piece_terms"] == T and plan["crossover"] == X
    is_long = lens > X
    short = np.where(is_long, 0, lens)
    npieces = (short + T - 1) // T
    assert plan["long_segments"] == int(is_long.sum())
    assert plan["short_terms"] == int(short.sum())
    assert plan["pieces"] == int(npieces.sum())
    assert plan["max_long"] == (int(lens[is_long].max()) if is_long.any() else 0)
    assert plan["workspace_bytes"] == workspace_bytes(n, n_seg, plan["pieces"], plan["short_terms"])
    first, ln, dest, desc = (plan[k].astype(np.int64) for k in ("piece_first", "piece_len", "piece_dest", "seg_desc"))
    # segment descriptors: first piece in segment order, piece count or the bucket-method mark
    starts = np.concatenate([[0], np.cumsum(npieces)])[:-1]
    assert np.array_equal(desc[:, 0], starts)
    assert np.array_equal(desc[:, 1], np.where(is_long, LONG, npieces))
    # pieces: lengths 1 .. T, longest first, the destinations a permutation
    if plan["pieces"]:
        assert ln.min() >= 1 and ln.max() <= T
        assert np.all(np.diff(ln) <= 0)
        assert np.array_equal(np.sort(dest), np.arange(plan["pieces"]))
        # piece `dest` of segment order is piece (dest - start) of its segment: it covers exactly those terms
        seg_of_piece = np.repeat(np.arange(n_seg), npieces)
        seg = seg_of_piece[dest]
        idx = dest - starts[seg]
        a = off[:-1].astype(np.int64)[seg] + idx * T
        assert np.array_equal(first, a)
        assert np.array_equal(ln, np.minimum(T, off[1:].astype(np.int64)[seg] - a))      # never across a segment border
    # every term in exactly one piece or one bucket-method segment
    cover = np.zeros(n + 1, dtype=np.int64)
    np.add.at(cover, first, 1)
    np.add.at(cover, first + ln, -1)
    lo, hi = off[:-1].astype(np.int64)[is_long], off[1:].astype(np.int64)[is_long]
    np.add.at(cover, lo, 1)
    np.add.at(cover, hi, -1)
    assert np.all(np.cumsum(cover)[:n] == 1)
    # runs of consecutive Straus terms: one more than the long segments at most
    assert plan["runs"] <= plan["long_segments"] + 1
    return plan


def test_random_offsets(S):
    rng = np.random.default_rng(1)
    for it in range(60):
        T = int(rng.choice([1, 2, 3, 8, 16, 64]))
        X = int(rng.choice([1, T, T + 1, 40, 300, 4096]))
        n_seg = int(rng.choice([1, 2, 63, 64, 65, 1000]))
        kind = it % 3
        if kind == 0:
            lens = rng.geometric(1.0 / (T + 2), size=n_seg) - 1
        elif kind == 1:
            lens = rng.choice([0, 1, T - 1, T, T + 1, 2 * T + 1, X - 1, X, X + 1, 2 * X + 1], size=n_seg)
        else:
            lens = rng.integers(0, 3 * X + 2, size=n_seg)
        check_plan(S, np.maximum(lens, 0), T, X)


def test_adversarial_offsets(S):
    T, X = 8, 4096
    check_plan(S, [0] * 5000, T, X)                                   # all empty
    check_plan(S, [0], T, X)
    check_plan(S, [1 << 20], T, X)                                    # one huge segment: the bucket method alone
    p = check_plan(S, [0, 0, 1 << 20, 0], T, X)
    assert p["pieces"] == 0 and p["runs"] == 0 and p["workspace_bytes"] == workspace_bytes(1 << 20, 4, 0, 0)
    p = check_plan(S, [1] * (1 << 20), T, X)                          # 2^20 segments of one term
    assert p["pieces"] == 1 << 20 and p["runs"] == 1
    for L in (T - 1, T, T + 1, X - 1, X, X + 1):
        check_plan(S, [L, 0, L, L], T, X)
    check_plan(S, [X + 1, 3, X + 1, X + 1, 0, 5, X + 7], T, X)        # Straus runs between bucket-method segments
    assert S.msm_segments_plan(3 * X, offsets_of([X] * 3), piece_terms=X, crossover=X, arrays=False)["piece_terms"] == 64   # capped


def test_defaults_follow_the_source(S, monkeypatch):
    """piece_terms == 0 / crossover == 0 select the compiled defaults when the environment overrides neither: the numbers
    DESIGN.md and the header quote are the ones in msm_seg.hip."""
    monkeypatch.delenv("S2K_MSM_SEG_T", raising=False)             # (the library reads them at every call)
    monkeypatch.delenv("S2K_MSM_SEG_CROSSOVER", raising=False)
    src = open(os.path.join(ROOT, "secp256k1_voi_amd", "csrc", "msm_seg.hip")).read()
    t = int(re.search(r"#define S2K_MSM_SEG_T (\d+)", src).group(1))
    x = int(re.search(r"#define S2K_MSM_SEG_CROSSOVER (\d+)", src).group(1))
    plan = S.msm_segments_plan(0, [0], arrays=False)
    assert (plan["piece_terms"], plan["crossover"]) == (t, x)
    assert 1 <= t <= 64
    # the carve restated above against the text it restates
    assert "carve(span * 2 * SEG_POS)" in src and "carve(span * SEG_TBL * SEG_ENTRY_BYTES)" in src
    assert "carve(p.piece_stride * SEG_PT_WORDS * 4)" in src and "carve(p.n_pieces * 12)" in src and "carve(n_seg * 8)" in src
    assert re.search(r"SEG_POS = 33;", src) and re.search(r"SEG_TBL = 8;", src) and "SEG_ENTRY_BYTES = 64, SEG_PT_WORDS = 27" in src


def test_sizes_are_refused_not_truncated(S):
    lib = S.load_library()
    summary = np.zeros(8, dtype=np.uint64)

    def plan_rc(n, off):
        o = np.asarray(off, dtype=np.uint64)
        return lib.s2k_debug_msm_segments_plan(n, len(off) - 1, o.ctypes.data, 0, 0, summary.ctypes.data, 0, None, None, None, None)

    assert plan_rc(MAX_TERMS, [0, MAX_TERMS]) == 0
    assert plan_rc(MAX_TERMS + 1, [0, MAX_TERMS + 1]) == ERR_ARG                      # above the limit of the single-sum call
    assert plan_rc((1 << 32) + 5, [0, (1 << 32) + 5]) == ERR_ARG                      # would be 5 terms in 32 bits
    assert plan_rc(5, [0, (1 << 32) + 5]) == ERR_ARG                                  # an offset above n
    assert plan_rc(5, [0, (1 << 32) + 2, 5]) == ERR_ARG                               # ... whose low 32 bits would pass
    assert plan_rc(5, [0, 1 << 63, 5]) == ERR_ARG
    for off in ([1, 5], [0, 3, 2, 5], [0, 4], [0, 6]):
        assert plan_rc(5, off) == ERR_ARG
    assert lib.s2k_debug_msm_segments_plan(0, 0, None, 0, 0, summary.ctypes.data, 0, None, None, None, None) == 0
    assert lib.s2k_debug_msm_segments_plan(3, 1, None, 0, 0, summary.ctypes.data, 0, None, None, None, None) == ERR_ARG
    assert lib.s2k_debug_msm_segments_plan(0, 0, None, 0, 0, None, 0, None, None, None, None) == ERR_ARG


def test_entry_points_refuse_without_a_device(S):
    """NULL context: S2K_ERR_ARG from both forms before anything touches a device (as test_cabi_cpu.py checks other entries)."""
    lib = S.load_library()
    k, p, out = np.zeros(64, np.uint8), np.zeros(130, np.uint8), np.zeros(65, np.uint8)
    off = np.asarray([0, 2], dtype=np.uint64)
    assert lib.s2k_multi_scalar_mult_segments(None, 2, k.ctypes.data, p.ctypes.data, 1, off.ctypes.data, out.ctypes.data) == ERR_ARG
    assert lib.s2k_multi_scalar_mult_segments_device(None, 2, None, None, 1, off.ctypes.data, None, None) == ERR_ARG
    assert not out.any()


def test_binding_checks_offsets_before_the_call(S):
    good = S.check_segment_offsets([0, 2, 2, 5], 5)
    assert good.dtype == np.uint64 and good.tolist() == [0, 2, 2, 5]
    for off, n in (([1, 5], 5), ([0, 3, 2, 5], 5), ([0, 4], 5), ([0, 6], 5), ([], 0), ([[0, 5]], 5), ([0, -1, 5], 5), ([0.0, 5.0], 5)):
        with pytest.raises(ValueError):
            S.check_segment_offsets(off, n)


def test_environment_overrides_are_read_per_call(S, monkeypatch):
    monkeypatch.setenv("S2K_MSM_SEG_T", "3")
    monkeypatch.setenv("S2K_MSM_SEG_CROSSOVER", "40")
    plan = check_plan(S, [0, 2, 3, 4, 40, 41, 7], 3, 40)
    got = S.msm_segments_plan(97, offsets_of([0, 2, 3, 4, 40, 41, 7]), arrays=False)
    assert (got["piece_terms"], got["crossover"], got["pieces"], got["long_segments"]) == (3, 40, plan["pieces"], 1)
    monkeypatch.setenv("S2K_MSM_SEG_T", "1000")                       # clamped to 1 .. 64
    assert S.msm_segments_plan(0, [0], arrays=False)["piece_terms"] == 64
