#!/usr/bin/env python3
"""Times s2k_multi_scalar_mult_segments_device against the two ways the library had before it, in ONE process with
device-resident inputs and HIP events.  Every shape: WARM warm-up rounds, then REPS (default 20) rounds of
[new, loop, loop2] alternated call by call, medians:

  new     one segmented call
  loop    a loop of s2k_multi_scalar_mult_device over the segments, twice (loop, loop2: their difference is the run-to-run
          spread of this run); with 2^12 segments or more only 256 of them are timed and the time is scaled (`scaled`)
  ladder  s2k_scalar_mult_batch on the same terms (the single-point ladder, n results instead of n_seg): HOST form - it has
          no device form - so its time includes the transfers of 97 bytes in and 65 bytes out per term; `new_host` is the
          segmented call's host form on the same input; wall clock, 2 warm-up rounds, REPS rounds alternated

then two sweeps over the segment length L = 2^8 .. 2^16, the segmented call with Straus forced against the same call with the
bucket method forced (S2K_MSM_SEG_CROSSOVER moved between calls, alternated): `crossover_total` at a fixed total of 2^20 terms
(2^20 / L segments: the sweep the default is read off) and `crossover_one` for ONE segment (latency); and, with --pieces, the
2^14 x 64 shape at several piece lengths.  Every JSON line names its own repetitions.
usage: msm_segments_time.py [--reps 20] [--quick] [--pieces] [--sweep-only] [--profile-shape LOG2_SEGMENTS]"""
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
ap.add_argument("--pieces", action="store_true", help="also sweep the piece length at 2^14 x 64")
ap.add_argument("--sweep-only", action="store_true", help="only the two crossover sweeps")
ap.add_argument("--profile-shape", type=int, default=None, metavar="LOG2_SEGMENTS",
                help="only five segmented calls of 2^LOG2_SEGMENTS equal segments, Straus forced (for a kernel-trace run)")
args = ap.parse_args()

eng = S.Engine(0, wait_tables=True)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
LOG_N = 16 if args.quick else 20
N = 1 << LOG_N
rng = np.random.default_rng(7)
d = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
d[:, 0] &= 0x7F
k = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
pts = eng.scalar_base_mult_batch(d)
dk, dp = torch.from_numpy(k).to(dev), torch.from_numpy(pts).to(dev)
dout = torch.zeros(N * 65 + 64, dtype=torch.uint8, device=dev)


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


def new_call(n, off):
    # the C entry point itself, as loop_call's: the binding's own offset checks (numpy, ~10 us) are done once, outside the timing
    off = S.check_segment_offsets(off, n)
    a_k, a_p, a_o, n_seg = dk.data_ptr(), dp.data_ptr(), dout.data_ptr(), off.shape[0] - 1

    def f():
        rc = eng._lib.s2k_multi_scalar_mult_segments_device(eng._h, n, a_k, a_p, n_seg, off.ctypes.data, a_o, st)
        assert rc == 0, rc
    return f


def loop_call(off, count):
    o = [int(x) for x in off[:count + 1]]
    a_k, a_p, a_o = dk.data_ptr(), dp.data_ptr(), dout.data_ptr()

    def f():
        for j in range(count):
            a, b = o[j], o[j + 1]
            rc = eng._lib.s2k_multi_scalar_mult_device(eng._h, b - a, a_k + 32 * a, a_p + 65 * a, a_o + 65 * j, st)
            assert rc == 0, rc
    return f


def emit(**kw):
    print(json.dumps(kw), flush=True)


def shape(n_seg, seg_len, ladder):
    n = n_seg * seg_len
    off = np.arange(n_seg + 1, dtype=np.uint64) * seg_len
    count = min(n_seg, 256) if n_seg >= 4096 else n_seg
    new, loop, loop2 = timed([new_call(n, off), loop_call(off, count), loop_call(off, count)])
    scale = n_seg / count
    row = dict(kind="shape", n_seg=n_seg, seg_len=seg_len, terms=n, reps=args.reps, warm=args.warm, new_ms=new, loop_ms=loop * scale,
               loop2_ms=loop2 * scale, scaled=count != n_seg, loop_segments_timed=count, ns_per_term_new=new * 1e6 / n)
    if ladder:
        fs = [lambda: eng.scalar_mult_batch(k[:n], pts[:n]), lambda: eng.multi_scalar_mult_segments(k[:n], pts[:n], off)]
        ts = [[], []]
        for r in range(2 + args.reps):
            for i, f in enumerate(fs):
                t0 = time.perf_counter()
                f()
                if r >= 2:
                    ts[i].append((time.perf_counter() - t0) * 1e3)
        row["ladder_host_ms"], row["new_host_ms"] = float(np.median(ts[0])), float(np.median(ts[1]))
        row["ns_per_item_ladder_host"] = row["ladder_host_ms"] * 1e6 / n
        row["ns_per_term_new_host"] = row["new_host_ms"] * 1e6 / n
    emit(**row)


def forced(n, off, crossover):
    f = new_call(n, off)

    def g():
        os.environ["S2K_MSM_SEG_CROSSOVER"] = str(crossover)
        try:
            f()
        finally:
            os.environ.pop("S2K_MSM_SEG_CROSSOVER")
    return g


def sweeps():
    for kind, total_log in (("crossover_total", LOG_N), ("crossover_one", None)):
        for lg in range(8, min(16, LOG_N) + 1):
            L = 1 << lg
            n_seg = 1 << (total_log - lg) if total_log is not None else 1
            off = np.arange(n_seg + 1, dtype=np.uint64) * L
            straus, bucket = timed([forced(n_seg * L, off, 1 << 30), forced(n_seg * L, off, 1)])
            emit(kind=kind, seg_len=L, n_seg=n_seg, reps=args.reps, warm=args.warm, straus_ms=straus, bucket_ms=bucket)


if args.profile_shape is not None:
    n_seg = 1 << args.profile_shape
    off = np.arange(n_seg + 1, dtype=np.uint64) * (N // n_seg)
    f = forced(N, off, 1 << 30)
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    emit(kind="profile_shape", n_seg=n_seg, seg_len=N // n_seg, calls=5)
    sys.exit(0)

emit(kind="config", log2_terms=LOG_N, reps=args.reps, warm=args.warm,
     **{k_: v for k_, v in S.msm_segments_plan(0, [0], arrays=False).items() if k_ in ("piece_terms", "crossover")})
if not args.sweep_only:
    for lg_seg in (16, 14, 12, 10, 6, 0):
        if lg_seg <= LOG_N:
            shape(1 << lg_seg, N >> lg_seg, ladder=lg_seg == 14)
    shape(64, 64, False)
    shape(1024, 64, False)
sweeps()
if args.pieces and not args.sweep_only:
    off = np.arange((N >> 6) + 1, dtype=np.uint64) * 64
    for T in (1, 2, 4, 8, 16, 32, 64):
        os.environ["S2K_MSM_SEG_T"] = str(T)
        ms, = timed([new_call(N, off)])
        emit(kind="piece_terms", piece_terms=T, n_seg=N >> 6, seg_len=64, reps=args.reps, warm=args.warm, new_ms=ms, ns_per_term=ms * 1e6 / N)
    os.environ.pop("S2K_MSM_SEG_T")
