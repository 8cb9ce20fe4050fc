"""Segmented multi-scalar multiplication (s2k_multi_scalar_mult_segments[_device]) on the GPU: every segment's record against
the CPU oracle (Straus per segment, or the base-point multiple of a known discrete logarithm), never against the engine's
own single-sum call alone.

On an MI355X the file takes about 30 s (19 tests)."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref as R
from pyref import b32

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENT = bytes(65)
ERR_ARG = -3                          # S2K_ERR_ARG


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
def T():
    import secp256k1_voi_amd as S
    return S.msm_segments_plan(0, [0], arrays=False)["piece_terms"]


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def expect_segments(oracle, ks, ps, lens):
    """oracle.multi_scalar_mult_vartime per segment, on reduced scalars (the oracle's Scalars are canonical)."""
    out, a = [], 0
    for L in lens:
        kr = [oracle.fn_reduce(k)[0] for k in ks[a:a + L]]
        out.append(oracle.multi_scalar_mult_vartime(kr, ps[a:a + L]) if L else IDENT)
        a += L
    return out


def run_segments(eng, ks, ps, lens):
    got = eng.multi_scalar_mult_segments(ks, ps, offsets_of(lens))
    assert got.shape == (len(lens), 65)
    return [bytes(r) for r in got]


def point_pool(oracle, rnd, count):
    return [oracle.scalar_base_mult_vartime(b32(rnd.randrange(1, R.N))) for _ in range(count)]


def random_terms(rnd, pool, count):
    return [b32(rnd.randrange(R.N)) for _ in range(count)], [pool[rnd.randrange(len(pool))] for _ in range(count)]


# ---- 1. small shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seg", [1, 2, 63, 64, 65, 1000])
def test_small_shapes(eng, oracle, T, n_seg):
    rnd = random.Random(7100 + n_seg)
    pool = point_pool(oracle, rnd, 16)
    full = [0, 1, 2, 3, max(T - 1, 0), T, T + 1, 2 * T + 1, 63, 64, 65, 255, 300]
    small = [0, 1, 2, 3, max(T - 1, 0), T, T + 1, 2 * T + 1]
    if n_seg == 1:
        shapes = [[L] for L in full]
    elif n_seg == 2:
        shapes = [[300, 0], [0, 65], [T + 1, 2 * T + 1], [1, 255]]
    else:
        lens = list(full) + [small[rnd.randrange(len(small))] for _ in range(n_seg - len(full) - 9)]
        rnd.shuffle(lens)
        mid = len(lens) // 2
        lens = [0, 0, 0] + lens[:mid] + [0, 0, 0] + lens[mid:] + [0, 0, 0]      # runs of empty segments: start, middle, end
        assert len(lens) == n_seg
        shapes = [lens]
    for lens in shapes:
        ks, ps = random_terms(rnd, pool, sum(lens))
        assert run_segments(eng, ks, ps, lens) == expect_segments(oracle, ks, ps, lens), lens[:20]


def test_no_terms_some_segments(eng):
    for n_seg in (1, 5, 300):
        got = eng.multi_scalar_mult_segments([], [], np.zeros(n_seg + 1, dtype=np.uint64))
        assert got.shape == (n_seg, 65) and not got.any()
    assert eng.multi_scalar_mult_segments([], [], [0]).shape == (0, 65)


# ---- 2. the edge pool of test_msm_edge_cases, in four placements -------------------------------------------------------
def edge_cases(oracle, rnd):
    P = point_pool(oracle, rnd, 8)
    negP0 = oracle.point_neg(P[0])
    lamP3 = b"\x04" + b32(R.BETA * int.from_bytes(P[3][1:33], "big") % R.P) + P[3][33:]      # lambda * P3 = (beta x, y)
    k2 = rnd.randrange(1, R.N)
    cases = [
        ([b32(5)] * 40, [P[0]] * 40),                                          # the same point 40 times
        ([b32(7), b32(7)], [P[0], negP0]),                                     # P and -P: identity
        ([b32(1), b32(R.N - 1)], [P[1], P[1]]),                                # k and n - k on one point: identity
        ([b32(0)] * 5, P[:5]),                                                 # zero scalars
        ([b32(3), b32(4)], [IDENT, P[2]]),                                     # an identity record
        ([b32(R.N - 1), b32(2**256 - 1), b32(R.N), b32(R.N + 1)], P[:4]),      # reduced as SetBytes does
        ([b32(sum(0xFFFF << (16 * i) for i in range(0, 16, 2))), b32(1 << 255)], P[4:6]),
        ([b32(1 << 128), b32((1 << 128) - 1)], P[6:8]),
        ([b32((R.N - k2 * R.LAMBDA) % R.N), b32(k2)], [P[3], lamP3]),          # P and lambda P, scalars that cancel
        ([b32(2), b32(R.N - 1), b32(R.N - 1)], [P[5], P[5], P[5]]),            # P + P inside the sum, then identity
    ]
    assert oracle.multi_scalar_mult_vartime(*cases[8]) == IDENT
    return P, cases


def test_edge_pool_placements(eng, oracle, T):
    rnd = random.Random(61)
    P, cases = edge_cases(oracle, rnd)
    for ck, cp in cases:
        # (a) a segment of its own, between two random neighbours
        ak, ap = random_terms(rnd, P, 3)
        bk, bp = random_terms(rnd, P, T + 2)
        for lens, ks, ps in (
            ([3, len(ck), T + 2], ak + ck + bk, ap + cp + bp),
            # (b) at the start of a segment (inside one piece when it has at most T terms), random terms behind it
            ([3, len(ck) + T + 2], ak + ck + bk, ap + cp + bp),
            # (c) straddling a piece border: T - 1 random terms in front of it
            ([max(T - 1, 1) + len(ck) + 3], bk[:max(T - 1, 1)] + ck + ak, bp[:max(T - 1, 1)] + cp + ap),
        ):
            assert run_segments(eng, ks, ps, lens) == expect_segments(oracle, ks, ps, lens), (len(ck), lens)
    # (d) every case as a single segment among 1000 random ones: the neighbours' results must not change
    lens = [rnd.randrange(0, 5) for _ in range(1000)]
    ks, ps = random_terms(rnd, P, sum(lens))
    base = expect_segments(oracle, ks, ps, lens)
    assert run_segments(eng, ks, ps, lens) == base
    offs = [0]
    for L in lens:
        offs.append(offs[-1] + L)
    where = sorted(rnd.sample(range(1001), len(cases)), reverse=True)
    lens2, ks2, ps2, exp2 = list(lens), list(ks), list(ps), list(base)
    for (ck, cp), at in zip(cases, where):          # back to front: earlier positions stay valid
        t = offs[at] if at < 1000 else offs[1000]
        lens2.insert(at, len(ck))
        ks2[t:t] = ck
        ps2[t:t] = cp
        exp2.insert(at, oracle.multi_scalar_mult_vartime([oracle.fn_reduce(k)[0] for k in ck], cp))
    assert run_segments(eng, ks2, ps2, lens2) == exp2


# ---- 3. large shapes by known discrete logarithms ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(eng):
    """2^20 terms as synth_msm_terms makes them (P_i = d_i G, scalars with a sprinkle of edge values), with the prefix sums of
    k_i d_i so that any segment's discrete logarithm is a difference."""
    n = 1 << 20
    rng = np.random.default_rng(2024)
    d = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d[:, 0] &= 0x7F
    d[:, 31] |= 1
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for j, v in enumerate([0, 1, R.N - 1, 1 << 128, (1 << 128) - 1, 0xFFFF << 64, R.N >> 1, 2**256 - 1, R.N]):
        for i in range(j * 7 + 3, n, n // 13 + j):
            k[i] = np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)
    pts = eng.scalar_base_mult_batch(d)
    kb, db = k.tobytes(), d.tobytes()
    pre = [0] * (n + 1)
    for i in range(n):
        pre[i + 1] = pre[i] + (int.from_bytes(kb[32 * i:32 * i + 32], "big") % R.N) * int.from_bytes(db[32 * i:32 * i + 32], "big")
    return k, pts, pre


def check_by_dlog(eng, oracle, big, lens):
    k, pts, pre = big
    off = offsets_of(lens)
    assert int(off[-1]) == k.shape[0]
    got = eng.multi_scalar_mult_segments(k, pts, off)
    bad = []
    for j in range(len(lens)):
        tot = (pre[int(off[j + 1])] - pre[int(off[j])]) % R.N
        exp = oracle.scalar_base_mult_vartime(b32(tot)) if tot else IDENT
        if bytes(got[j]) != exp:
            bad.append(j)
    assert not bad, (len(bad), bad[:10])
    return got


@pytest.mark.parametrize("n_seg,seg_len", [(1 << 14, 64), (1 << 10, 1024), (1 << 16, 16)])
def test_large_uniform(eng, oracle, big, n_seg, seg_len):
    check_by_dlog(eng, oracle, big, [seg_len] * n_seg)


def ragged_lens(total, seed, mean, long_len=0, empties=0):
    rng = np.random.default_rng(seed)
    lens, left = [], total - long_len
    while left > 0:
        L = min(int(rng.geometric(1.0 / mean)), left)
        lens.append(L)
        left -= L
    if long_len:
        lens.insert(len(lens) // 2, long_len)
    for _ in range(empties):
        lens.insert(int(rng.integers(0, len(lens) + 1)), 0)
    return lens


def test_large_ragged_with_one_bucket_segment(eng, oracle, big):
    import secp256k1_voi_amd as S
    lens = [0, 0] + ragged_lens(1 << 20, 5, 24, long_len=1 << 18, empties=200) + [0]
    plan = S.msm_segments_plan(1 << 20, offsets_of(lens), arrays=False)
    assert plan["long_segments"] >= 1 and plan["pieces"] > 0          # both paths in one call
    check_by_dlog(eng, oracle, big, lens)


def test_one_segment_of_everything(eng, oracle, big):
    k, pts, _ = big
    got = check_by_dlog(eng, oracle, big, [1 << 20])
    assert bytes(got[0]) == eng.multi_scalar_mult(k, pts)              # the same code path: byte for byte


# ---- 4. drop-in for a loop of single sums --------------------------------------------------------------------------------
def test_equals_loop_of_single_sums(eng, big):
    k, pts, _ = big
    lens = ragged_lens(1 << 16, 11, 16, empties=300)
    lens = lens[:1 << 12] if len(lens) >= 1 << 12 else lens
    while len(lens) < 1 << 12:
        lens.append(len(lens) % 40)
    n = sum(lens)
    off = offsets_of(lens)
    got = eng.multi_scalar_mult_segments(k[:n], pts[:n], off)
    for j in range(len(lens)):
        a, b = int(off[j]), int(off[j + 1])
        assert bytes(got[j]) == eng.multi_scalar_mult(k[a:b], pts[a:b]), j


# ---- 5. errors; the device form ------------------------------------------------------------------------------------------
def test_errors(eng, oracle):
    import ctypes
    import secp256k1_voi_amd as S
    rnd = random.Random(5)
    P = point_pool(oracle, rnd, 4)
    ks, ps = random_terms(rnd, P, 10)
    for off in ([1, 10], [0, 6, 5, 10], [0, 5, 9], [0, 5, 11], [], [0, -1, 10]):
        with pytest.raises(ValueError):
            eng.multi_scalar_mult_segments(ks, ps, off)
    with pytest.raises(ValueError):
        eng.multi_scalar_mult_segments(ks, ps[:9], [0, 10])             # length mismatch (the reference panics)
    # the same through the C-ABI itself: S2K_ERR_ARG, nothing written
    lib = eng._lib
    kk, pp = np.frombuffer(b"".join(ks), np.uint8), np.frombuffer(b"".join(ps), np.uint8)
    out = np.full(3 * 65, 0xAB, dtype=np.uint8)
    for off in ([1, 5, 10], [0, 6, 5, 10], [0, 5, 9], [0, 5, 11]):
        o = np.asarray(off, dtype=np.uint64)
        assert lib.s2k_multi_scalar_mult_segments(eng._h, 10, kk.ctypes.data, pp.ctypes.data, len(off) - 1, o.ctypes.data, out.ctypes.data) == ERR_ARG
        assert (out == 0xAB).all()
    o = np.asarray([0, 10], dtype=np.uint64)
    assert lib.s2k_multi_scalar_mult_segments(eng._h, 10, None, pp.ctypes.data, 1, o.ctypes.data, out.ctypes.data) == ERR_ARG
    assert lib.s2k_multi_scalar_mult_segments(eng._h, 10, kk.ctypes.data, None, 1, o.ctypes.data, out.ctypes.data) == ERR_ARG
    assert lib.s2k_multi_scalar_mult_segments(eng._h, 10, kk.ctypes.data, pp.ctypes.data, 1, o.ctypes.data, None) == ERR_ARG
    assert lib.s2k_multi_scalar_mult_segments(eng._h, 10, kk.ctypes.data, pp.ctypes.data, 1, None, out.ctypes.data) == ERR_ARG
    assert lib.s2k_multi_scalar_mult_segments_device(eng._h, 10, None, None, 1, o.ctypes.data, None, None) == ERR_ARG
    # a malformed record in segment 500 of 1000
    lens = [rnd.randrange(1, 4) for _ in range(1000)]
    ks, ps = random_terms(rnd, P, sum(lens))
    assert run_segments(eng, ks, ps, lens) == expect_segments(oracle, ks, ps, lens)
    at = sum(lens[:500])
    bad = bytearray(ps[at]); bad[64] ^= 1
    ps[at] = bytes(bad)
    with pytest.raises(S.EngineError):
        eng.multi_scalar_mult_segments(ks, ps, offsets_of(lens))
    ps[at] = b"\x02" + ps[at][1:]                                      # neither 0x04 nor the identity record
    with pytest.raises(S.EngineError):
        eng.multi_scalar_mult_segments(ks, ps, offsets_of(lens))


def test_device_form_on_caller_stream(eng, big):
    import torch
    k, pts, _ = big
    lens = ragged_lens(40000, 3, 20, long_len=20000, empties=20)       # one segment on the bucket method
    n, off = sum(lens), offsets_of(lens)
    host = eng.multi_scalar_mult_segments(k[:n], pts[:n], off)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        dk, dp = torch.from_numpy(k[:n]).to(dev), torch.from_numpy(pts[:n]).to(dev)
        out = torch.full((len(lens) * 65 + 64,), 0xCD, dtype=torch.uint8, device=dev)
        stream.synchronize()
        eng.multi_scalar_mult_segments_device(n, dk.data_ptr(), dp.data_ptr(), off, out.data_ptr(), stream.cuda_stream)
        got = out.cpu().numpy()
    assert np.array_equal(got[:len(lens) * 65].reshape(-1, 65), host)
    assert (got[len(lens) * 65:] == 0xCD).all()                        # nothing written behind the records


# ---- 6. both sides of the crossover and of the piece length, on small inputs ------------------------------------------
@pytest.mark.parametrize("env", [{"S2K_MSM_SEG_T": "3", "S2K_MSM_SEG_CROSSOVER": "40"},
                                 {"S2K_MSM_SEG_T": "1", "S2K_MSM_SEG_CROSSOVER": "2"},
                                 {"S2K_MSM_SEG_T": "64", "S2K_MSM_SEG_CROSSOVER": "100000"}])
def test_small_piece_length_and_crossover(env):
    """Tests 1 and 2 once more in a child process whose environment moves the piece length and the crossover: segments of
    63 .. 300 terms take the bucket method and short ones are several pieces (first two), or nothing takes the bucket method
    and a lane holds up to 64 terms (third)."""
    e = dict(os.environ)
    e.update(env)
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-k", "test_small_shapes or test_edge_pool_placements or test_no_terms_some_segments"],
                       env=e, capture_output=True, text=True, timeout=1500, cwd=ROOT)
    assert p.returncode == 0 and " passed" in p.stdout and " skipped" not in p.stdout, p.stdout[-3000:] + p.stderr[-1500:]
