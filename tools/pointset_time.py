#!/usr/bin/env python3
"""Times s2k_pointset_multi_scalar_mult_segments_device against s2k_multi_scalar_mult_segments_device on the same terms (the
points expanded from the set: the only way to do this work without a point set), in ONE process with device-resident inputs
and HIP events.  Every shape: WARM warm-up rounds, then REPS (default 20) rounds of [set at 8 bits, set at 4 bits, segmented
call] alternated call by call, medians:

  dense    2^14 x 64, 2^16 x 16, 2^10 x 1024 and 64 x 64: the term at position t of its segment uses point t of a set of
           seg_len points
  indexed  2^14 x 64 with random indices into a set of 2^12 points

then the time to create a set of 64 and of 2^12 points at both widths (wall clock, the call synchronises), the piece-length
sweep at 2^14 x 64 (S2K_POINTSET_T moved between calls) and the crossover sweep: segments of 2^8 .. 2^16 terms at a fixed total
of 2^20, the set's own path forced against the gathered bucket method forced (S2K_POINTSET_CROSSOVER moved between calls,
alternated; indices into the 2^12-point set).  Every JSON line names its own repetitions.
usage: pointset_time.py [--reps 20] [--quick] [--no-sweeps] [--profile WIDTH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import secp256k1_voi_amd as S

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="2^16 terms instead of 2^20 (a functional check of the tool)")
ap.add_argument("--no-sweeps", action="store_true", help="only the shapes and the creation times")
ap.add_argument("--profile", type=int, default=None, metavar="WIDTH",
                help="only five point-set calls (WIDTH 4 or 8) or five segmented calls (WIDTH 0) at 2^14 x 64 dense (for a kernel-trace run)")
args = ap.parse_args()

eng = S.Engine(0, wait_tables=True)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
LOG_N = 16 if args.quick else 20
N = 1 << LOG_N
rng = np.random.default_rng(9)
M_MAX = 1 << 12
d = rng.integers(0, 256, size=(M_MAX, 32), dtype=np.uint8)
d[:, 0] &= 0x7F
d[:, 31] |= 1
base = eng.scalar_base_mult_batch(d)                      # the points every set here is a prefix of
k = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
dk = torch.from_numpy(k).to(dev)
dout = torch.zeros(N * 65 + 64, dtype=torch.uint8, device=dev)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fs, reps=args.reps, warm=args.warm):
    """medians (ms) of the callables in fs, alternated call by call"""
    for _ in range(warm):
        for f in fs:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fs]
    for _ in range(reps):
        for i, f in enumerate(fs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [float(np.median(t)) for t in ts]


def set_call(ps, n, off, d_idx):
    # the C entry point itself: the binding's own offset checks (numpy) are done once, outside the timing
    off = S.check_segment_offsets(off, n)
    a_k, a_i, a_o, n_seg = dk.data_ptr(), (d_idx.data_ptr() if d_idx is not None else None), dout.data_ptr(), off.shape[0] - 1

    def f():
        rc = eng._lib.s2k_pointset_multi_scalar_mult_segments_device(eng._h, ps._k, n, a_k, a_i, n_seg, off.ctypes.data, a_o, st)
        assert rc == 0, rc
    return f


def seg_call(n, off, d_pts):
    off = S.check_segment_offsets(off, n)
    a_k, a_p, a_o, n_seg = dk.data_ptr(), d_pts.data_ptr(), dout.data_ptr(), off.shape[0] - 1

    def f():
        rc = eng._lib.s2k_multi_scalar_mult_segments_device(eng._h, n, a_k, a_p, n_seg, off.ctypes.data, a_o, st)
        assert rc == 0, rc
    return f


def with_env(f, name, value):
    def g():
        os.environ[name] = str(value)
        try:
            f()
        finally:
            os.environ.pop(name)
    return g


def shape(kind, n_seg, seg_len, m):
    n = n_seg * seg_len
    off = np.arange(n_seg + 1, dtype=np.uint64) * seg_len
    if kind == "dense":
        idx = np.tile(np.arange(seg_len, dtype=np.uint32), n_seg)
        d_idx = None
    else:
        idx = rng.integers(0, m, size=n, dtype=np.uint32)
        d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
    d_pts = torch.from_numpy(base[:m][idx]).to(dev)       # the expanded point array the segmented call takes
    ps8, ps4 = eng.pointset_create(base[:m], 8), eng.pointset_create(base[:m], 4)
    try:
        f8, f4, fs = set_call(ps8, n, off, d_idx), set_call(ps4, n, off, d_idx), seg_call(n, off, d_pts)
        # all three give the same records
        outs = []
        for f in (f8, f4, fs):
            f()
            outs.append(dout[:n_seg * 65].cpu().numpy().copy())
        assert np.array_equal(outs[0], outs[2]) and np.array_equal(outs[1], outs[2])
        t8, t4, ts = timed([f8, f4, fs])
        emit(kind=kind, n_seg=n_seg, seg_len=seg_len, terms=n, set_points=m, reps=args.reps, warm=args.warm, set8_ms=t8, set4_ms=t4,
             segments_ms=ts, ratio8=ts / t8, ratio4=ts / t4, ns_per_term_set8=t8 * 1e6 / n, set8_bytes=ps8.device_bytes(), set4_bytes=ps4.device_bytes())
    finally:
        ps8.close()
        ps4.close()


def creation(m):
    for c in (8, 4):
        ts = []
        for r in range(1 + 5):
            t0 = time.perf_counter()
            ps = eng.pointset_create(base[:m], c)
            if r:
                ts.append((time.perf_counter() - t0) * 1e3)
            nbytes = ps.device_bytes()
            ps.close()
        emit(kind="create", set_points=m, window_bits=c, reps=5, warm=1, create_ms=float(np.median(ts)), device_bytes=nbytes)


SEGS, LEN = (N >> 6), 64
if args.profile is not None:
    off = np.arange(SEGS + 1, dtype=np.uint64) * LEN
    if args.profile:
        ps = eng.pointset_create(base[:LEN], args.profile)
        f = set_call(ps, N, off, None)
    else:
        d_pts = torch.from_numpy(base[:LEN][np.tile(np.arange(LEN, dtype=np.uint32), SEGS)]).to(dev)
        f = seg_call(N, off, d_pts)
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    emit(kind="profile", window_bits=args.profile, n_seg=SEGS, seg_len=LEN, calls=5)
    sys.exit(0)

emit(kind="config", log2_terms=LOG_N, reps=args.reps, warm=args.warm, piece_terms=int(os.environ.get("S2K_POINTSET_T", 8)),
     crossover=int(os.environ.get("S2K_POINTSET_CROSSOVER", 16384)))
shape("dense", SEGS, LEN, LEN)
shape("dense", N >> 4, 16, 16)
shape("dense", N >> 10, 1024, 1024)
shape("dense", 64, 64, 64)
shape("indexed", SEGS, LEN, M_MAX)
creation(64)
creation(M_MAX)
if not args.no_sweeps:
    ps8 = eng.pointset_create(base[:LEN], 8)
    off = np.arange(SEGS + 1, dtype=np.uint64) * LEN
    f = set_call(ps8, N, off, None)
    for T in (1, 2, 4, 8, 16, 32, 64):
        ms, = timed([with_env(f, "S2K_POINTSET_T", T)])
        emit(kind="piece_terms", window_bits=8, piece_terms=T, n_seg=SEGS, seg_len=LEN, reps=args.reps, warm=args.warm, set8_ms=ms, ns_per_term=ms * 1e6 / N)
    ps8.close()
    ps8 = eng.pointset_create(base, 8)
    d_idx = torch.from_numpy(rng.integers(0, M_MAX, size=N, dtype=np.uint32).view(np.int32)).to(dev)
    for lg in range(8, min(16, LOG_N) + 1):
        L = 1 << lg
        n_seg = N >> lg
        off = np.arange(n_seg + 1, dtype=np.uint64) * L
        f = set_call(ps8, N, off, d_idx)
        own, bucket = timed([with_env(f, "S2K_POINTSET_CROSSOVER", 1 << 30), with_env(f, "S2K_POINTSET_CROSSOVER", 1)])
        emit(kind="crossover_total", window_bits=8, seg_len=L, n_seg=n_seg, reps=args.reps, warm=args.warm, set_ms=own, bucket_ms=bucket)
    ps8.close()
