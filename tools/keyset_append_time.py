#!/usr/bin/env python3
"""Times growing a key set against rebuilding it, and verification over a grown set against a set created whole, in ONE
process, the variants alternated call by call; medians (with min and max) of REPS rounds.  A COMB and a JOINT5 set of 2^16
keys, each with an index.

  a   KeySet.append of K keys (K = 1, 64, 4096) into a set of 2^16 keys created with a capacity of 2^16 + 4096 and an index:
      wall clock of the synchronous call, host key bytes in, tables and index complete at its end.  Every round appends to a
      fresh set (its creation is not timed), so every append starts from 2^16 keys.
  b   the only route without the call: keyset_create over all 2^16 + K keys plus index_create, wall clock.
  c   2^20 signatures over all 2^16 + 4096 keys, device-resident (HIP events around the _device forms): by index and fused by
      key bytes, over the set grown by (a) with K = 4096 (`grown`), over a set created whole from the same keys (`whole`) and
      over one created whole with a quarter more capacity than keys (`spare`).  Spare capacity and the way the set came to be
      must cost a call nothing: two variants agree when their medians differ by less than the runs' own min-max spread
      (`agree` in the line).

One JSON line per layout and K for a / b (with b / a), one per layout for c.

usage: keyset_append_time.py [--reps 9] [--warm 2] [--n 1048576] [--keys 65536] [--spare 4096] [--layouts COMB,JOINT5]
                             [--out profiles/r19_keyset_append_time.jsonl]"""
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
ap.add_argument("--appends", default="1,64,4096")
ap.add_argument("--layouts", default="COMB,JOINT5")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_keyset_append_time.jsonl"))
args = ap.parse_args()
N, NKEYS, SPARE = args.n, args.keys, args.spare
CAP = NKEYS + SPARE
KS = [int(x) for x in args.appends.split(",")]
assert KS[-1] == max(KS) <= SPARE

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


# the batch: N valid signatures over all CAP keys (signature i under key i mod CAP)
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, N, CAP, seed=1901))
keys = np.ascontiguousarray(pub[:CAP])
assert len(np.unique(keys, axis=0)) == CAP
kidx = (np.arange(N) % CAP).astype(np.uint32)
d_pub, d_dig, d_r, d_s = (torch.from_numpy(x).to(dev) for x in (pub, dig, r, s))
d_kidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
d_val = torch.zeros(N, dtype=torch.uint8, device=dev)

for name in args.layouts.split(","):
    layout = getattr(S, "KEYSET_" + name)

    def grown(k):
        ks = eng.keyset_create(keys[:NKEYS], layout, capacity=CAP)
        ks.index_create()
        return ks

    def rebuilt(k):
        ks = eng.keyset_create(keys[:NKEYS + k], layout)
        ks.index_create()
        return ks

    last = None
    for k in KS:
        a_ms, b_ms = [], []
        for rep in range(args.warm + args.reps):
            ks = grown(k)
            ms, first = wall(lambda: ks.append(keys[NKEYS:NKEYS + k]))
            assert first == NKEYS and len(ks) == NKEYS + k
            if k == KS[-1] and rep == args.warm + args.reps - 1:
                last = ks                                   # (the grown set of part c)
            else:
                ks.close()
            ms_b, whole = wall(lambda: rebuilt(k))
            whole.close()
            if rep >= args.warm:
                a_ms.append(ms)
                b_ms.append(ms_b)
        A, B = summary(a_ms), summary(b_ms)
        emit(what="keyset_append", layout=name, keys=NKEYS, capacity=CAP, appended=k, reps=args.reps, append=A, rebuild=B,
             rebuild_over_append=round(B["ms"] / A["ms"], 1))

    # c: verification over the grown set and over one created whole
    g = last
    assert len(g) == CAP == g.capacity()
    w = eng.keyset_create(keys, layout)
    w.index_create()
    sp = eng.keyset_create(keys, layout, capacity=CAP + CAP // 4)
    sp.index_create()
    assert len(sp) == CAP and sp.device_bytes() > w.device_bytes()
    assert g.device_bytes() == w.device_bytes() and g.index_info()["occupied"] == w.index_info()["occupied"] == CAP
    p = [x.data_ptr() for x in (d_dig, d_r, d_s)]
    variants = {
        "index_grown": lambda: eng.ecdsa_verify_batch_keyset_device(g, N, d_kidx.data_ptr(), *p, d_val.data_ptr(), stream=st),
        "index_whole": lambda: eng.ecdsa_verify_batch_keyset_device(w, N, d_kidx.data_ptr(), *p, d_val.data_ptr(), stream=st),
        "index_spare": lambda: eng.ecdsa_verify_batch_keyset_device(sp, N, d_kidx.data_ptr(), *p, d_val.data_ptr(), stream=st),
        "fused_grown": lambda: eng.ecdsa_verify_batch_bykey_device(g, N, d_pub.data_ptr(), *p, d_val.data_ptr(), stream=st),
        "fused_whole": lambda: eng.ecdsa_verify_batch_bykey_device(w, N, d_pub.data_ptr(), *p, d_val.data_ptr(), stream=st),
        "fused_spare": lambda: eng.ecdsa_verify_batch_bykey_device(sp, N, d_pub.data_ptr(), *p, d_val.data_ptr(), stream=st),
    }
    for kname, f in variants.items():                       # every variant accepts the batch, all of it on the set's tables
        d_val.zero_()
        f()
        torch.cuda.synchronize()
        assert int(d_val.sum().item()) == N, kname
        assert eng.key_grouping_stats()["keyed"] == N, kname
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
    D = {kname: summary(m) for kname, m in zip(variants, ms)}

    def agree(x, y):
        spread = max(D[x]["max"] - D[x]["min"], D[y]["max"] - D[y]["min"])
        return abs(D[x]["ms"] - D[y]["ms"]) <= spread
    emit(what="keyset_append_verify", layout=name, n=N, keys=CAP, grown_from=NKEYS, reps=max(args.reps, 15), device=D,
         index_grown_minus_whole_ms=round(D["index_grown"]["ms"] - D["index_whole"]["ms"], 4),
         fused_grown_minus_whole_ms=round(D["fused_grown"]["ms"] - D["fused_whole"]["ms"], 4),
         index_spare_minus_whole_ms=round(D["index_spare"]["ms"] - D["index_whole"]["ms"], 4),
         fused_spare_minus_whole_ms=round(D["fused_spare"]["ms"] - D["fused_whole"]["ms"], 4),
         agree={"index_grown": agree("index_grown", "index_whole"), "fused_grown": agree("fused_grown", "fused_whole"),
                "index_spare": agree("index_spare", "index_whole"), "fused_spare": agree("fused_spare", "fused_whole")})
    sp.close()
    g.close()
    w.close()
eng.close()
out_f.close()
