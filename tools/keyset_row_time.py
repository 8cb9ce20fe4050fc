#!/usr/bin/env python3
"""Times small key-set calls by size, in ONE process, the variants alternated call by call; medians of REPS rounds.
A JOINT5 set of 1024 keys; n = 64 .. 8192 signatures; ECDSA and BIP-340.

  a  the key-set call on the wave-per-signature ladder over the set's tables (k_verify_row_keyset / k_schnorr_row_keyset;
     s2k_ctx_set_keyset_small_batch_max above n)
  b  the same call with the setting at 0: the lane-per-signature key-set path (scalar preparation, generator part, sort,
     ladder, worklist kernel)
  c  the plain s2k_ecdsa_verify_batch / s2k_schnorr_verify_batch call on the expanded keys (k_verify_row / k_schnorr_row up to
     s2k_ctx_set_small_batch_max, the four-lane ladders above)

Device-resident (HIP events around the _device form) and host to host (wall clock around the host form).  One JSON line per
size and algorithm, then one line with the threshold the figures yield: the largest measured n at which a is below b by more
than b's own spread over its repeats (max - min of the device-resident times), in both algorithms, capped at 3072; 0 if none.

usage: keyset_row_time.py [--reps 15] [--sizes 64,256,...] [--keys 1024]"""
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
from secp256k1_voi_amd.synth import synth_batch, synth_schnorr_batch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--sizes", default="64,256,1024,2048,3072,4096,8192")
ap.add_argument("--keys", type=int, default=1024)
ap.add_argument("--layout", type=int, default=S.KEYSET_JOINT5)
args = ap.parse_args()
SIZES = [int(x) for x in args.sizes.split(",")]
NMAX = max(SIZES)

eng = S.Engine(0, wait_tables=True)
lib, h = eng._lib, eng._h
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
ROW_DEFAULT = 3072


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed_events(fs):
    for _ in range(args.warm):
        for f in fs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fs]
    for _ in range(args.reps):
        for j, f in enumerate(fs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[j].append(a.elapsed_time(b))
    return ms


def timed_wall(fs):
    for _ in range(args.warm):
        for f in fs:
            f()
    ms = [[] for _ in fs]
    for _ in range(args.reps):
        for j, f in enumerate(fs):
            t0 = time.perf_counter()
            f()
            ms[j].append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def with_row(max_n, f):
    def g():
        eng.set_keyset_small_batch_max(max_n)
        r = f()
        assert eng.last_keyset_ladder() == (S.KEYSET_LADDER_ROW if max_n else S.KEYSET_LADDER_LANE)
        return r
    return g


results = {}

# ---- ECDSA ----
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, NMAX, args.keys, seed=1401))
keys, inv = np.unique(pub, axis=0, return_inverse=True)
kidx = inv.reshape(-1).astype(np.uint32)
ks = eng.keyset_create(keys, args.layout)
dpub, ddig, dr, ds = (torch.from_numpy(x).to(dev) for x in (pub, dig, r, s))
dkidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
dval = torch.zeros(NMAX, dtype=torch.uint8, device=dev)
for n in SIZES:
    dev_call = lambda: eng.ecdsa_verify_batch_keyset_device(ks, n, dkidx.data_ptr(), ddig.data_ptr(), dr.data_ptr(), ds.data_ptr(), dval.data_ptr(), stream=st)
    plain_dev = lambda: eng.ecdsa_verify_batch_device(n, dpub.data_ptr(), ddig.data_ptr(), dr.data_ptr(), ds.data_ptr(), dval.data_ptr(), stream=st)
    fs = [with_row(1 << 20, dev_call), with_row(0, dev_call), plain_dev]
    for f in fs:                                      # every variant accepts the synthetic batch
        dval.zero_()
        f()
        torch.cuda.synchronize()
        assert int(dval[:n].sum().item()) == n
    dms = timed_events(fs)
    host_call = lambda: eng.ecdsa_verify_batch_keyset(ks, kidx[:n], dig[:n], r[:n], s[:n])
    plain_host = lambda: eng.ecdsa_verify_batch(pub[:n], dig[:n], r[:n], s[:n])
    hms = timed_wall([with_row(1 << 20, host_call), with_row(0, host_call), plain_host])
    row = {"what": "ecdsa", "n": n, "keys": len(keys), "layout": ks.layout(), "reps": args.reps,
           "device": {k: summary(m) for k, m in zip("abc", dms)}, "host": {k: summary(m) for k, m in zip("abc", hms)}}
    results[("ecdsa", n)] = row
    emit(**row)
ks.close()

# ---- BIP-340 ----
pk, msgs, sig = (np.ascontiguousarray(x) for x in synth_schnorr_batch(eng, NMAX, args.keys, seed=1402))
xs, inv = np.unique(pk, axis=0, return_inverse=True)
pts65, okd = eng.point_decode_batch(np.concatenate([np.full((len(xs), 1), 2, np.uint8), xs], axis=1), 33)
assert bool(okd.all())
xkeys = np.ascontiguousarray(pts65[:, 1:])
odd = np.arange(len(xkeys)) % 2 == 1                     # every other key with the OTHER y: the sign flip of the ladder at work
P_FIELD = 2**256 - 2**32 - 977
xkeys[odd, 32:] = np.frombuffer(b"".join((P_FIELD - int.from_bytes(bytes(y), "big")).to_bytes(32, "big") for y in xkeys[odd, 32:]),
                                np.uint8).reshape(-1, 32)
kidx = inv.reshape(-1).astype(np.uint32)
ks = eng.keyset_create(xkeys, args.layout)
dpk, dmsg, dsig = (torch.from_numpy(x).to(dev) for x in (pk, msgs, sig))
dkidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
for n in SIZES:
    dev_call = lambda: eng.schnorr_verify_batch_keyset_device(ks, n, dkidx.data_ptr(), dmsg.data_ptr(), 32, dsig.data_ptr(), dval.data_ptr(), st)

    def plain_dev():
        assert lib.s2k_schnorr_verify_batch_device(h, n, dpk.data_ptr(), dmsg.data_ptr(), None, 32, dsig.data_ptr(), 0, dval.data_ptr(), st) == 0
    fs = [with_row(1 << 20, dev_call), with_row(0, dev_call), plain_dev]
    for f in fs:
        dval.zero_()
        f()
        torch.cuda.synchronize()
        assert int(dval[:n].sum().item()) == n
    dms = timed_events(fs)
    host_call = lambda: eng.schnorr_verify_batch_keyset(ks, kidx[:n], msgs[:n], sig[:n])
    plain_host = lambda: eng.schnorr_verify_batch(pk[:n], msgs[:n], sig[:n])
    hms = timed_wall([with_row(1 << 20, host_call), with_row(0, host_call), plain_host])
    row = {"what": "schnorr", "n": n, "keys": len(xkeys), "layout": ks.layout(), "reps": args.reps,
           "device": {k: summary(m) for k, m in zip("abc", dms)}, "host": {k: summary(m) for k, m in zip("abc", hms)}}
    results[("schnorr", n)] = row
    emit(**row)
ks.close()
eng.set_keyset_small_batch_max(ROW_DEFAULT)


def wins(row):
    a, b = row["device"]["a"], row["device"]["b"]
    return b["ms"] - a["ms"] > b["max"] - b["min"]


good = [n for n in SIZES if all(wins(results[(w, n)]) for w in ("ecdsa", "schnorr"))]
emit(what="threshold", rule="largest n where a < b by more than b's max - min, both algorithms, capped at 3072",
     sizes_where_row_wins=good, largest=max(good) if good else 0, default=min(max(good), 3072) if good else 0)
eng.close()
