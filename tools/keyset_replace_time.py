#!/usr/bin/env python3
"""Times replacing keys of a key set in place against appending as many and against rebuilding the set, and verification over
a set after 4096 replacements against a set created whole from the same list, in ONE process, the variants alternated call
by call; medians (with min and max) of REPS rounds.  A COMB and a JOINT5 set of 2^16 keys, each with an index.

Every round starts from a fresh set of 2^16 keys with room for 4096 more, then, for m = 1, 64, 4096 (one m per round):
  d   what a caller must do without the call: destroy the set, keyset_create of the whole list and index_create (wall clock),
  e   of which the index build alone (index_create),
  c   the yardstick - KeySet.append of m keys into the spare capacity: the same table kernels built in place, the index grown,
  a   KeySet.replace of m scattered slots (a fixed permutation),
  b   KeySet.replace of m adjacent slots.
The expectation to confirm or explain: a = b = c + e + the scatter's own time (`a_minus_c_minus_e` in the line; the scatter
kernel's time comes from a kernel trace of this tool in a run of its own).
Then 2^20 signatures by index, device-resident (HIP events), over the set after 4096 replacements (`replaced`) and over a set
created whole from the same list (`whole`): they agree when their medians differ by less than the runs' own min-max spread.

One JSON line per layout and m, one per layout for the verification.

usage: keyset_replace_time.py [--reps 9] [--warm 2] [--n 1048576] [--keys 65536] [--spare 4096] [--counts 1,64,4096]
                              [--layouts COMB,JOINT5] [--out profiles/r22_keyset_replace_time.jsonl]"""
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
from secp256k1_voi_amd.synth import synth_batch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=1 << 16)
ap.add_argument("--spare", type=int, default=4096)
ap.add_argument("--counts", default="1,64,4096")
ap.add_argument("--layouts", default="COMB,JOINT5")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_keyset_replace_time.jsonl"))
args = ap.parse_args()
N, NKEYS, SPARE = args.n, args.keys, args.spare
CAP = NKEYS + SPARE
MS = [int(x) for x in args.counts.split(",")]
M = max(MS)
assert MS[-1] == M == SPARE and 2 * M <= NKEYS and N >= CAP     # (the last round fills the capacity: the set of the verification)

eng = S.Engine(0, wait_tables=True)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
out_f = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out_f.write(line + "\n")
    out_f.flush()


def summary(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def random_keys(count, seed):
    d = np.random.default_rng(seed).integers(0, 256, size=(count, 32), dtype=np.uint8)
    d[:, 0] &= 0x7F
    d[:, 31] |= 1
    return np.ascontiguousarray(eng.scalar_base_mult_batch(d)[:, 1:])


# the final key list and N valid signatures over it (signature i under row i mod CAP); the set starts with other keys in the
# rows that get replaced, so that the batch verifies only once every replacement has arrived
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, N, CAP, seed=2201))
final = np.ascontiguousarray(pub[:CAP])
assert len(np.unique(final, axis=0)) == CAP
kidx = (np.arange(N) % CAP).astype(np.uint32)
scattered = np.sort(np.random.default_rng(2202).permutation(NKEYS - M)[:M] + M).astype(np.uint32)    # rows M .. NKEYS - 1
scattered = scattered[np.random.default_rng(2203).permutation(M)]                                     # (given out of order)
adjacent = np.arange(M, dtype=np.uint32)                                                              # rows 0 .. M - 1
start = final.copy()
other = random_keys(2 * M, 2204)
start[scattered] = other[:M]
start[adjacent] = other[M:]
d_dig, d_r, d_s = (torch.from_numpy(x).to(dev) for x in (dig, r, s))
d_kidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
d_val = torch.zeros(N, dtype=torch.uint8, device=dev)

for name in args.layouts.split(","):
    layout = getattr(S, "KEYSET_" + name)
    ks = None
    for m in MS:
        T = {k: [] for k in "abcde"}
        for rep in range(args.warm + args.reps):
            def rebuild():
                if ks is not None:
                    ks.close()
                return eng.keyset_create(start[:NKEYS], layout, capacity=CAP)
            ms_create, ks = wall(rebuild)
            ms_index, _ = wall(ks.index_create)
            put = (final, start)[rep % 2]                   # (every call changes the rows it names)
            k_c, k_a, k_b = (np.ascontiguousarray(x) for x in (start[NKEYS:NKEYS + m], put[scattered[:m]], put[adjacent[:m]]))
            ms_c, first = wall(lambda: ks.append(k_c))
            ms_a, _ = wall(lambda: ks.replace(scattered[:m], k_a))
            ms_b, _ = wall(lambda: ks.replace(adjacent[:m], k_b))
            assert first == NKEYS and len(ks) == NKEYS + m
            if rep >= args.warm:
                for k, v in zip("abcde", (ms_a, ms_b, ms_c, ms_create + ms_index, ms_index)):
                    T[k].append(v)
        A, B, Cc, D, E = (summary(T[k]) for k in "abcde")
        emit(what="keyset_replace", layout=name, keys=NKEYS, capacity=CAP, m=m, reps=args.reps, replace_scattered=A, replace_adjacent=B,
             append=Cc, rebuild=D, index_create=E, a_minus_c_minus_e=round(A["ms"] - Cc["ms"] - E["ms"], 4),
             append_spread=round(Cc["max"] - Cc["min"], 4), rebuild_over_replace=round(D["ms"] / A["ms"], 1))

    # verification over the set after M replacements and over one created whole from the same list
    g = ks
    assert len(g) == CAP == g.capacity()
    g.replace(scattered, final[scattered])
    g.replace(adjacent, final[adjacent])
    w = eng.keyset_create(final, layout, capacity=CAP)
    w.index_create()
    assert g.device_bytes() == w.device_bytes() and g.index_info()["occupied"] == w.index_info()["occupied"] == CAP
    p = [x.data_ptr() for x in (d_dig, d_r, d_s)]
    variants = {
        "replaced": lambda: eng.ecdsa_verify_batch_keyset_device(g, N, d_kidx.data_ptr(), *p, d_val.data_ptr(), stream=st),
        "whole": lambda: eng.ecdsa_verify_batch_keyset_device(w, N, d_kidx.data_ptr(), *p, d_val.data_ptr(), stream=st),
    }
    for kname, f in variants.items():                       # both accept the whole batch: every replacement arrived
        d_val.zero_()
        f()
        torch.cuda.synchronize()
        assert int(d_val.sum().item()) == N, kname
    fs = list(variants.values())
    for _ in range(args.warm + 1):
        for f in fs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fs]
    for _ in range(max(args.reps, 15)):
        for j, f in enumerate(fs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[j].append(e0.elapsed_time(e1))
    D = {kname: summary(v) for kname, v in zip(variants, ms)}
    spread = max(D["replaced"]["max"] - D["replaced"]["min"], D["whole"]["max"] - D["whole"]["min"])
    emit(what="keyset_replace_verify", layout=name, n=N, keys=CAP, replaced=2 * M, reps=max(args.reps, 15), device=D,
         replaced_minus_whole_ms=round(D["replaced"]["ms"] - D["whole"]["ms"], 4), agree=abs(D["replaced"]["ms"] - D["whole"]["ms"]) <= spread)
    g.close()
    w.close()
eng.close()
out_f.close()
