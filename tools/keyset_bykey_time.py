#!/usr/bin/env python3
"""Times ECDSA verification of a batch given as KEY BYTES against a long-lived key set, in ONE process, the variants alternated
call by call; medians (with min and max) of REPS rounds after WARM warm-ups.  2^20 signatures over 2^16 keys, a JOINT5 and a
COMB set, each with an index (KeySet.index_create).

  a  the plain ecdsa_verify_batch[_device] call on the key bytes: groups the batch and builds comb tables inside every call - the
     only way to verify such a batch without the index, the baseline
  b  the by-index key-set call on the same set (the caller has resolved the indices somehow: not counted)
  c  the fused call by key bytes, every key in the set (s2k_ecdsa_verify_batch_keyset_bykey[_device])
  d  the fused call with 1/16 of the signatures under keys outside the set (the general ladder for those)
  e  keyset_lookup_device alone (device-resident only)

Device-resident (HIP events around the _device forms) and host to host (wall clock around the host forms).  One JSON line per
layout with c/a and c - b; then, per layout, mid-size calls (2^13 and 2^15 signatures) with the small- and mid-batch
thresholds forced off - a_off and c_off - beside the plain call as shipped (a_default: what the fused call delegates to below
s2k_ctx_set_mid_batch_max).

usage: keyset_bykey_time.py [--reps 15] [--warm 3] [--n 1048576] [--keys 65536] [--out profiles/r15_keyset_bykey_time.jsonl]"""
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
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=1 << 16)
ap.add_argument("--mid", default="8192,32768")
ap.add_argument("--layouts", default="JOINT5,COMB")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_keyset_bykey_time.jsonl"))
args = ap.parse_args()
N, NKEYS = args.n, args.keys
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768

eng = S.Engine(0, wait_tables=True)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
out_f = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out_f.write(line + "\n")
    out_f.flush()


def timed(fs, events):
    for _ in range(args.warm):
        for f in fs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fs]
    for _ in range(args.reps):
        for j, f in enumerate(fs):
            if events:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[j].append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                f()
                ms[j].append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


# the batch: N valid signatures of NKEYS keys; its variant with every 16th signature under a key the set does not hold
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, N, NKEYS, seed=1501))
keys, inv = np.unique(pub, axis=0, return_inverse=True)
kidx = inv.reshape(-1).astype(np.uint32)
n_out = N // 16
opub, odig, orr, oss = (np.ascontiguousarray(x) for x in synth_batch(eng, n_out, max(NKEYS // 16, 1), seed=1502))
pub2, dig2, r2, s2 = pub.copy(), dig.copy(), r.copy(), s.copy()
pub2[::16], dig2[::16], r2[::16], s2[::16] = opub[:len(pub2[::16])], odig[:len(pub2[::16])], orr[:len(pub2[::16])], oss[:len(pub2[::16])]
d1 = [torch.from_numpy(x).to(dev) for x in (pub, dig, r, s)]
d2 = [torch.from_numpy(x).to(dev) for x in (pub2, dig2, r2, s2)]
dkidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
dfound = torch.zeros(N, dtype=torch.int32, device=dev)
dval = torch.zeros(N, dtype=torch.uint8, device=dev)
p1, p2 = [x.data_ptr() for x in d1], [x.data_ptr() for x in d2]

for name in args.layouts.split(","):
    t0 = time.perf_counter()
    ks = eng.keyset_create(keys, getattr(S, "KEYSET_" + name))
    t1 = time.perf_counter()
    ks.index_create()
    t2 = time.perf_counter()
    info = ks.index_info()
    eng.set_small_batch_max(ROW_DEFAULT)
    eng.set_mid_batch_max(QUAD_DEFAULT)
    fa = lambda n=N: eng.ecdsa_verify_batch_device(n, *p1, dval.data_ptr(), stream=st)
    fb = lambda n=N: eng.ecdsa_verify_batch_keyset_device(ks, n, dkidx.data_ptr(), *p1[1:], dval.data_ptr(), stream=st)
    fc = lambda n=N: eng.ecdsa_verify_batch_bykey_device(ks, n, *p1, dval.data_ptr(), stream=st)
    fd = lambda n=N: eng.ecdsa_verify_batch_bykey_device(ks, n, *p2, dval.data_ptr(), stream=st)
    fe = lambda n=N: eng.keyset_lookup_device(ks, n, p1[0], dfound.data_ptr(), stream=st)
    stats = {}
    for k, f in zip("abcd", (fa, fb, fc, fd)):            # every variant accepts the synthetic batch; hits and misses as planned
        dval.zero_()
        f()
        torch.cuda.synchronize()
        assert int(dval.sum().item()) == N, k
        stats[k] = eng.key_grouping_stats()
    assert stats["c"]["keyed"] == N and stats["c"]["general"] == 0 and stats["d"]["general"] == len(pub2[::16]), stats
    fe()
    torch.cuda.synchronize()
    assert bool((dfound == dkidx).all().item())
    dms = timed([fa, fb, fc, fd, fe], events=True)
    ha = lambda: eng.ecdsa_verify_batch(pub, dig, r, s)
    hb = lambda: eng.ecdsa_verify_batch_keyset(ks, kidx, dig, r, s)
    hc = lambda: eng.ecdsa_verify_batch_bykey(ks, pub, dig, r, s)
    hd = lambda: eng.ecdsa_verify_batch_bykey(ks, pub2, dig2, r2, s2)
    hms = timed([ha, hb, hc, hd], events=False)
    D = {k: summary(m) for k, m in zip("abcde", dms)}
    H = {k: summary(m) for k, m in zip("abcd", hms)}
    emit(what="bykey", layout=name, n=N, keys=len(keys), reps=args.reps, set_build_s=round(t1 - t0, 3), index_build_s=round(t2 - t1, 4),
         index=info, device=D, host=H,
         device_c_over_a=round(D["c"]["ms"] / D["a"]["ms"], 4), device_c_minus_b_ms=round(D["c"]["ms"] - D["b"]["ms"], 4),
         device_a_spread_ms=round(D["a"]["max"] - D["a"]["min"], 4),
         host_c_over_a=round(H["c"]["ms"] / H["a"]["ms"], 4), host_c_minus_b_ms=round(H["c"]["ms"] - H["b"]["ms"], 4))
    # mid-size calls: the fused lane path against the plain call, thresholds forced off; and the plain call as shipped
    for n in [int(x) for x in args.mid.split(",")]:
        def off(f):
            def g():
                eng.set_small_batch_max(0)
                eng.set_mid_batch_max(0)
                f(n)
            return g

        def shipped(f):
            def g():
                eng.set_small_batch_max(ROW_DEFAULT)
                eng.set_mid_batch_max(QUAD_DEFAULT)
                f(n)
            return g
        mms = timed([off(fa), off(fc), shipped(fa)], events=True)
        emit(what="bykey_mid", layout=name, n=n, keys=len(keys), reps=args.reps,
             device={k: summary(m) for k, m in zip(("a_off", "c_off", "a_default"), mms)})
    eng.set_small_batch_max(ROW_DEFAULT)
    eng.set_mid_batch_max(QUAD_DEFAULT)
    ks.close()
eng.close()
out_f.close()
