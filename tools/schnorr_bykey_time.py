#!/usr/bin/env python3
"""Times BIP-340 verification of a batch given as X-ONLY KEY BYTES against a long-lived key set, in ONE process, the variants
alternated call by call; medians (with min and max) of REPS rounds after WARM warm-ups.  2^20 signatures of 32-byte messages
over 2^16 keys, a JOINT5 and a COMB set, each with an index (KeySet.index_create).

Device-resident (HIP events around the _device forms):
  a   the plain s2k_schnorr_verify_batch_device call on the key bytes: groups the batch and builds comb tables inside every call
  b   the by-index key-set call on the same set (the caller has resolved the indices somehow: not counted)
  b2  s2k_keyset_lookup_device with key_bytes 32, then the by-index call: the two-call route
  c   the fused call by key bytes, every key in the set (s2k_schnorr_verify_batch_keyset_bykey_device)
  d   the fused call with 1/16 of the signatures under keys outside the set (the general ladder for those)
Host to host from page-locked memory (wall clock), per 2^20 signatures: the synchronous forms of a, b and c, then four tickets in
flight - the fused BIP-340 call against the by-index BIP-340 ticket (the plain BIP-340 call has no ticket form), and the fused
ECDSA call against the plain and the by-index ECDSA tickets.
One JSON line per layout with c / a, c - b and c - b2; then, per layout, mid-size calls (2^13 and 2^15 signatures) with the
small- and mid-batch thresholds forced off - a_off and c_off - beside the plain call as shipped (a_default: what the fused call
delegates to below s2k_ctx_set_mid_batch_max).

usage: schnorr_bykey_time.py [--reps 15] [--warm 3] [--n 1048576] [--keys 65536] [--out profiles/r17_schnorr_bykey_time.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import pyref as R
import secp256k1_voi_amd as S
from secp256k1_voi_amd.synth import synth_batch, synth_schnorr_batch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=1 << 16)
ap.add_argument("--mid", default="8192,32768")
ap.add_argument("--layouts", default="JOINT5,COMB")
ap.add_argument("--tickets", type=int, default=12, help="tickets per timed run of a submit form (four in flight)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_schnorr_bykey_time.jsonl"))
args = ap.parse_args()
N, NKEYS = args.n, args.keys
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768

eng = S.Engine(0, wait_tables=True)
lib, h = eng._lib, eng._h
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


def lifted(xs):
    """X || Y rows of x-only keys, every other one stored with odd y"""
    out = np.zeros((len(xs), 64), np.uint8)
    for j, x in enumerate(xs):
        pt = R.lift_x(int.from_bytes(bytes(x), "big"), j & 1)
        out[j] = np.frombuffer(R.b32(pt[0]) + R.b32(pt[1]), np.uint8)
    return out


def pinned(a):
    p = S.pinned_array(a.shape, a.dtype)
    p[...] = a
    return p


# the batch: N valid signatures of NKEYS keys; its variant with every 16th signature under a key the set does not hold
pk, msgs, sig = (np.ascontiguousarray(x) for x in synth_schnorr_batch(eng, N, NKEYS, seed=1701))
xs, inv = np.unique(pk, axis=0, return_inverse=True)
keys = lifted(xs)
kidx = inv.reshape(-1).astype(np.uint32)
n_out = len(pk[::16])
opk, omsgs, osig = (np.ascontiguousarray(x) for x in synth_schnorr_batch(eng, n_out, max(NKEYS // 16, 1), seed=1702))
pk2, msgs2, sig2 = pk.copy(), msgs.copy(), sig.copy()
pk2[::16], msgs2[::16], sig2[::16] = opk, omsgs, osig
d1 = [torch.from_numpy(x).to(dev) for x in (pk, msgs, sig)]
d2 = [torch.from_numpy(x).to(dev) for x in (pk2, msgs2, sig2)]
dkidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
dfound = torch.zeros(N, dtype=torch.int32, device=dev)
dval = torch.zeros(N, dtype=torch.uint8, device=dev)
p1, p2 = [x.data_ptr() for x in d1], [x.data_ptr() for x in d2]
hpk, hmsgs, hsig, hkidx = pinned(pk), pinned(msgs), pinned(sig), pinned(kidx)
# the ECDSA batch of the ticket rows
epub, edig, er, es = (pinned(np.ascontiguousarray(x)) for x in synth_batch(eng, N, NKEYS, seed=1703))
ekeys, einv = np.unique(epub, axis=0, return_inverse=True)
ekidx = pinned(einv.reshape(-1).astype(np.uint32))


def in_flight(submit):
    """args.tickets tickets, four in flight; ms per batch"""
    def run():
        tk = []
        for j in range(args.tickets):
            if j >= 4:
                tk[j - 4].wait()
            tk.append(submit())
        for t in tk[-4:]:
            t.wait()
    def f():
        t0 = time.perf_counter()
        run()
        return (time.perf_counter() - t0) * 1e3 / args.tickets
    return f


for name in args.layouts.split(","):
    t0 = time.perf_counter()
    ks = eng.keyset_create(keys, getattr(S, "KEYSET_" + name))
    t1 = time.perf_counter()
    ks.index_create()
    t2 = time.perf_counter()
    info = ks.index_info()
    eng.set_small_batch_max(ROW_DEFAULT)
    eng.set_mid_batch_max(QUAD_DEFAULT)

    def fa(n=N):
        assert lib.s2k_schnorr_verify_batch_device(h, n, p1[0], p1[1], None, 32, p1[2], 0, dval.data_ptr(), st) == 0
    fb = lambda n=N: eng.schnorr_verify_batch_keyset_device(ks, n, dkidx.data_ptr(), p1[1], 32, p1[2], dval.data_ptr(), stream=st)

    def fb2(n=N):
        eng.keyset_lookup_device(ks, n, p1[0], dfound.data_ptr(), key_bytes=32, stream=st)
        eng.schnorr_verify_batch_keyset_device(ks, n, dfound.data_ptr(), p1[1], 32, p1[2], dval.data_ptr(), stream=st)
    fc = lambda n=N: eng.schnorr_verify_batch_bykey_device(ks, n, p1[0], p1[1], 32, p1[2], dval.data_ptr(), stream=st)
    fd = lambda n=N: eng.schnorr_verify_batch_bykey_device(ks, n, p2[0], p2[1], 32, p2[2], dval.data_ptr(), stream=st)
    stats = {}
    for k, f in zip(("a", "b", "b2", "c", "d"), (fa, fb, fb2, fc, fd)):     # every variant accepts the synthetic batch; hits and misses as planned
        dval.zero_()
        f()
        torch.cuda.synchronize()
        assert int(dval.sum().item()) == N, k
        stats[k] = eng.key_grouping_stats()
    assert stats["c"]["keyed"] == N and stats["c"]["general"] == 0 and stats["d"]["general"] == n_out, stats
    dms = timed([fa, fb, fb2, fc, fd], events=True)
    D = {k: summary(m) for k, m in zip(("a", "b", "b2", "c", "d"), dms)}
    # host to host from page-locked memory: synchronous, then four tickets in flight
    ha = lambda: eng.schnorr_verify_batch(hpk, hmsgs, hsig)
    hb = lambda: eng.schnorr_verify_batch_keyset(ks, hkidx, hmsgs, hsig)
    hc = lambda: eng.schnorr_verify_batch_bykey(ks, hpk, hmsgs, hsig)
    assert int(hc().sum()) == N
    hms = timed([ha, hb, hc], events=False)
    H = {k: summary(m) for k, m in zip(("a", "b", "c"), hms)}
    eks = eng.keyset_create(ekeys, getattr(S, "KEYSET_" + name))
    eks.index_create()
    assert int(eng.ecdsa_verify_batch_bykey_submit(eks, epub, edig, er, es).wait().sum()) == N
    assert int(eng.schnorr_verify_batch_bykey_submit(ks, hpk, hmsgs, hsig).wait().sum()) == N
    subs = {"schnorr_b": in_flight(lambda: eng.schnorr_verify_batch_keyset_submit(ks, hkidx, hmsgs, hsig)),
            "schnorr_c": in_flight(lambda: eng.schnorr_verify_batch_bykey_submit(ks, hpk, hmsgs, hsig)),
            "ecdsa_a": in_flight(lambda: eng.ecdsa_verify_batch_submit(epub, edig, er, es)),
            "ecdsa_b": in_flight(lambda: eng.ecdsa_verify_batch_keyset_submit(eks, ekidx, edig, er, es)),
            "ecdsa_c": in_flight(lambda: eng.ecdsa_verify_batch_bykey_submit(eks, epub, edig, er, es))}
    for f in subs.values():
        f()
    tms = {k: [] for k in subs}
    for _ in range(max(args.reps // 3, 3)):
        for k, f in subs.items():
            tms[k].append(f())
    eng.wait_all()
    eks.close()
    T = {k: summary(m) for k, m in tms.items()}
    emit(what="schnorr_bykey", layout=name, n=N, keys=len(keys), reps=args.reps, set_build_s=round(t1 - t0, 3), index_build_s=round(t2 - t1, 4),
         index=info, device=D, host_sync=H, host_tickets=T, tickets_per_run=args.tickets,
         device_c_over_a=round(D["c"]["ms"] / D["a"]["ms"], 4), device_c_minus_b_ms=round(D["c"]["ms"] - D["b"]["ms"], 4),
         device_c_minus_b2_ms=round(D["c"]["ms"] - D["b2"]["ms"], 4), device_b2_spread_ms=round(D["b2"]["max"] - D["b2"]["min"], 4),
         host_c_over_a=round(H["c"]["ms"] / H["a"]["ms"], 4))
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
        emit(what="schnorr_bykey_mid", layout=name, n=n, keys=len(keys), reps=args.reps,
             device={k: summary(m) for k, m in zip(("a_off", "c_off", "a_default"), mms)})
    eng.set_small_batch_max(ROW_DEFAULT)
    eng.set_mid_batch_max(QUAD_DEFAULT)
    ks.close()
eng.close()
out_f.close()
