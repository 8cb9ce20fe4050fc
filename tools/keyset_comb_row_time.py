#!/usr/bin/env python3
"""Times small calls over a COMB key set, in ONE process, the variants alternated call by call; medians of REPS rounds with
min - max.  A comb set of 1024 keys and a JOINT5 set of the same keys; ECDSA and BIP-340.

  a  the key-set call on the wave-per-signature ladder over the comb tables (k_verify_row_comb / k_schnorr_row_comb;
     s2k_ctx_set_keyset_comb_small_batch_max above n)
  b  the same call with that setting at 0: the lane-per-signature key-set path (scalar preparation, generator part, sort,
     k_verify_comb, finish / worklist kernels) - what a comb set's small call took before, and still takes by default
  c  the plain s2k_ecdsa_verify_batch / s2k_schnorr_verify_batch call on the expanded keys (k_verify_row / k_schnorr_row)
  d  the chunk-table row ladder over the JOINT5 set (k_verify_row_keyset / k_schnorr_row_keyset)

All four at --at (1024) signatures; a against b at every size of --sizes.  Device-resident (HIP events around the _device
form) and host to host (wall clock around the host form).  One JSON line per size and algorithm, then one line with the
crossover the figures yield: the largest measured n up to which a is below b by more than b's own spread over its repeats
(max - min of the device-resident times) at every measured size, in both algorithms; 0 if none.

usage: keyset_comb_row_time.py [--reps 15] [--sizes 256,512,...] [--at 1024] [--keys 1024]"""
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
ap.add_argument("--sizes", default="256,512,1024,2048,3072,4096,8192")
ap.add_argument("--at", type=int, default=1024)
ap.add_argument("--keys", type=int, default=1024)
args = ap.parse_args()
SIZES = sorted(set(int(x) for x in args.sizes.split(",")) | {args.at})
NMAX = max(SIZES)

eng = S.Engine(0, wait_tables=True)
lib, h = eng._lib, eng._h
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
CHUNK_ROW_DEFAULT = 2048


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


def with_comb_row(max_n, f):
    def g():
        eng.set_keyset_comb_small_batch_max(max_n)
        r = f()
        assert eng.last_keyset_ladder() == (S.KEYSET_LADDER_ROW_COMB if max_n else S.KEYSET_LADDER_LANE)
        return r
    return g


def with_chunk_row(f):
    def g():
        eng.set_keyset_small_batch_max(1 << 20)
        r = f()
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_ROW
        return r
    return g


def measure(what, n, dev_fs, host_fs, names, dval, keys):
    for f in dev_fs:                                  # every variant accepts the synthetic batch
        dval.zero_()
        f()
        torch.cuda.synchronize()
        assert int(dval[:n].sum().item()) == n
    dms, hms = timed_events(dev_fs), timed_wall(host_fs)
    row = {"what": what, "n": n, "keys": keys, "reps": args.reps,
           "device": {k: summary(m) for k, m in zip(names, dms)}, "host": {k: summary(m) for k, m in zip(names, hms)}}
    emit(**row)
    return row


results = {}
dval = torch.zeros(NMAX, dtype=torch.uint8, device=dev)

# ---- ECDSA ----
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, NMAX, args.keys, seed=2101))
keys, inv = np.unique(pub, axis=0, return_inverse=True)
kidx = inv.reshape(-1).astype(np.uint32)
ks, kj = eng.keyset_create(keys, S.KEYSET_COMB), eng.keyset_create(keys, S.KEYSET_JOINT5)
dpub, ddig, dr, ds = (torch.from_numpy(x).to(dev) for x in (pub, dig, r, s))
dkidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
for n in SIZES:
    set_dev = lambda k: (lambda: eng.ecdsa_verify_batch_keyset_device(k, n, dkidx.data_ptr(), ddig.data_ptr(), dr.data_ptr(), ds.data_ptr(), dval.data_ptr(), stream=st))
    set_host = lambda k: (lambda: eng.ecdsa_verify_batch_keyset(k, kidx[:n], dig[:n], r[:n], s[:n]))
    dev_fs = [with_comb_row(1 << 20, set_dev(ks)), with_comb_row(0, set_dev(ks))]
    host_fs = [with_comb_row(1 << 20, set_host(ks)), with_comb_row(0, set_host(ks))]
    if n == args.at:
        dev_fs += [lambda: eng.ecdsa_verify_batch_device(n, dpub.data_ptr(), ddig.data_ptr(), dr.data_ptr(), ds.data_ptr(), dval.data_ptr(), stream=st),
                   with_chunk_row(set_dev(kj))]
        host_fs += [lambda: eng.ecdsa_verify_batch(pub[:n], dig[:n], r[:n], s[:n]), with_chunk_row(set_host(kj))]
    results[("ecdsa", n)] = measure("ecdsa", n, dev_fs, host_fs, "abcd", dval, len(keys))
ks.close()
kj.close()

# ---- BIP-340 ----
pk, msgs, sig = (np.ascontiguousarray(x) for x in synth_schnorr_batch(eng, NMAX, args.keys, seed=2102))
xs, inv = np.unique(pk, axis=0, return_inverse=True)
pts65, okd = eng.point_decode_batch(np.concatenate([np.full((len(xs), 1), 2, np.uint8), xs], axis=1), 33)
assert bool(okd.all())
xkeys = np.ascontiguousarray(pts65[:, 1:])
odd = np.arange(len(xkeys)) % 2 == 1                     # every other key with the OTHER y: the sign flip of the ladder at work
P_FIELD = 2**256 - 2**32 - 977
xkeys[odd, 32:] = np.frombuffer(b"".join((P_FIELD - int.from_bytes(bytes(y), "big")).to_bytes(32, "big") for y in xkeys[odd, 32:]),
                                np.uint8).reshape(-1, 32)
kidx = inv.reshape(-1).astype(np.uint32)
ks, kj = eng.keyset_create(xkeys, S.KEYSET_COMB), eng.keyset_create(xkeys, S.KEYSET_JOINT5)
dpk, dmsg, dsig = (torch.from_numpy(x).to(dev) for x in (pk, msgs, sig))
dkidx = torch.from_numpy(kidx.view(np.int32)).to(dev)
for n in SIZES:
    set_dev = lambda k: (lambda: eng.schnorr_verify_batch_keyset_device(k, n, dkidx.data_ptr(), dmsg.data_ptr(), 32, dsig.data_ptr(), dval.data_ptr(), st))
    set_host = lambda k: (lambda: eng.schnorr_verify_batch_keyset(k, kidx[:n], msgs[:n], sig[:n]))

    def plain_dev():
        assert lib.s2k_schnorr_verify_batch_device(h, n, dpk.data_ptr(), dmsg.data_ptr(), None, 32, dsig.data_ptr(), 0, dval.data_ptr(), st) == 0
    dev_fs = [with_comb_row(1 << 20, set_dev(ks)), with_comb_row(0, set_dev(ks))]
    host_fs = [with_comb_row(1 << 20, set_host(ks)), with_comb_row(0, set_host(ks))]
    if n == args.at:
        dev_fs += [plain_dev, with_chunk_row(set_dev(kj))]
        host_fs += [lambda: eng.schnorr_verify_batch(pk[:n], msgs[:n], sig[:n]), with_chunk_row(set_host(kj))]
    results[("schnorr", n)] = measure("schnorr", n, dev_fs, host_fs, "abcd", dval, len(xkeys))
ks.close()
kj.close()
eng.set_keyset_comb_small_batch_max(0)
eng.set_keyset_small_batch_max(CHUNK_ROW_DEFAULT)


def wins(row):
    a, b = row["device"]["a"], row["device"]["b"]
    return b["ms"] - a["ms"] > b["max"] - b["min"]


good = []
for n in SIZES:                                        # (from the smallest size up, without a gap)
    if not all(wins(results[(w, n)]) for w in ("ecdsa", "schnorr")):
        break
    good.append(n)
at = {w: results[(w, args.at)]["device"] for w in ("ecdsa", "schnorr")}
emit(what="crossover", rule="largest measured n up to which a < b by more than b's max - min at every size, both algorithms",
     sizes_where_comb_row_wins=good, crossover=max(good) if good else 0,
     claim_at=args.at, claim_holds={w: bool(wins(results[(w, args.at)])) for w in ("ecdsa", "schnorr")},
     a_over_d_at={w: round(at[w]["a"]["ms"] / at[w]["d"]["ms"], 3) for w in at})
eng.close()
