#!/usr/bin/env python3
"""Times the SHA-2 digest kernel and the ECDSA verification calls that take messages against their digest siblings, in ONE
process, the variants alternated call by call; medians (with min and max) of REPS rounds after WARM warm-ups.

  host_hash  BEFORE the device is touched: the time 16 worker processes take to hash the 2^20 messages with hashlib (threads
             would not do: hashlib keeps the GIL for short inputs), wall clock around the whole map - what a Python caller of
             the digest forms pays first - and the slowest worker's own loop, without the hand-over of the results
  a          k_digest_messages alone (s2k_digest_batch_device), 2^20 items of 32, 64 and 250 bytes, per algorithm, resident
  b          s2k_ecdsa_verify_messages_batch_device against s2k_ecdsa_verify_batch_device on the same signatures (2^20 over
             2^16 keys, 32-byte messages, SHA-256): the plain call, and a JOINT5 key set by key bytes
  c          the same host to host from page-locked memory, synchronous and as four tickets in flight (per batch)
  d          a 1024-item synchronous call from messages against the digest call

usage: messages_time.py [--reps 11] [--warm 3] [--n 1048576] [--keys 65536] [--out profiles/r23_messages_time.jsonl]"""
import argparse
import hashlib
import json
import multiprocessing as mp
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=1 << 16)
ap.add_argument("--workers", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_messages_time.jsonl"))
args = ap.parse_args()
N, NKEYS, W = args.n, args.keys, args.workers
LENS = (32, 64, 250)
HASHES = {"sha256": lambda m: hashlib.sha256(m).digest(), "sha256d": lambda m: hashlib.sha256(hashlib.sha256(m).digest()).digest(),
          "sha512": lambda m: hashlib.sha512(m).digest()}

rng = np.random.default_rng(2301)
MSGS = {L: rng.integers(0, 256, size=(N, L), dtype=np.uint8) for L in LENS}      # (the workers inherit these)


def hash_slice(job):
    name, L, lo, hi = job
    f, mv = HASHES[name], memoryview(MSGS[L]).cast("B")
    t0 = time.perf_counter()
    out = b"".join(f(mv[i * L:(i + 1) * L]) for i in range(lo, hi))
    return out, time.perf_counter() - t0


def summary(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


out_f = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out_f.write(line + "\n")
    out_f.flush()


# ---- host hashing, before the device is touched (the workers are forked from a process that holds no GPU) ----
host_hash, digest32 = {}, None
with mp.get_context("fork").Pool(W) as pool:
    per = (N + W - 1) // W
    for name, L in (("sha256", 32), ("sha256d", 32), ("sha512", 32), ("sha256", 64), ("sha256", 250)):
        jobs = [(name, L, lo, min(N, lo + per)) for lo in range(0, N, per)]
        wall, inner = [], []
        for it in range(args.warm + args.reps):
            t0 = time.perf_counter()
            res = pool.map(hash_slice, jobs)
            blob = b"".join(r[0] for r in res)
            t1 = time.perf_counter()
            if it >= args.warm:
                wall.append((t1 - t0) * 1e3)
                inner.append(max(r[1] for r in res) * 1e3)
        host_hash[f"{name}_{L}"] = {"wall": summary(wall), "slowest_worker_loop": summary(inner)}
        if (name, L) == ("sha256", 32):
            digest32 = np.frombuffer(blob, np.uint8).reshape(N, 32).copy()
emit(what="host_hash", n=N, workers=W, cpus=os.cpu_count(), reps=args.reps, ms=host_hash)

import torch                                                   # noqa: E402
import secp256k1_voi_amd as S                                  # noqa: E402
from secp256k1_voi_amd.synth import synth_batch               # noqa: E402

eng = S.Engine(0, wait_tables=True)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
ALGS = {"sha256": S.HASH_SHA256, "sha256d": S.HASH_SHA256D, "sha512": S.HASH_SHA512}


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


# ---- (a) the digest kernel alone, device-resident ----
dmsgs = {L: torch.from_numpy(MSGS[L]).to(dev) for L in LENS}
dout = torch.zeros(N * 64, dtype=torch.uint8, device=dev)
names, fs = [], []
for name, alg in ALGS.items():
    for L in LENS:
        out_len = 64 if name == "sha512" else 32
        f = (lambda alg=alg, L=L, out_len=out_len: eng.digest_batch_device(alg, N, dmsgs[L].data_ptr(), None, L, dout.data_ptr(), out_len, stream=st))
        f()
        torch.cuda.synchronize()
        got = dout[:1000 * out_len].cpu().numpy().reshape(1000, out_len)
        assert all(bytes(got[i]) == HASHES[name](bytes(MSGS[L][i])) for i in range(1000)), (name, L)
        names.append(f"{name}_{L}")
        fs.append(f)
ams = timed(fs, events=True)
emit(what="a_digest_kernel", n=N, reps=args.reps, device={k: summary(m) for k, m in zip(names, ams)})

# ---- the signatures: valid over SHA-256 of the 32-byte messages ----
msgs = MSGS[32]
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, N, NKEYS, seed=2302, digest=digest32))
keys = np.unique(pub, axis=0)
ks = eng.keyset_create(keys, S.KEYSET_JOINT5)
ks.index_create()
d = {k: torch.from_numpy(x).to(dev) for k, x in (("pub", pub), ("dig", dig), ("r", r), ("s", s), ("msgs", msgs))}
p = {k: v.data_ptr() for k, v in d.items()}
dval = torch.zeros(N, dtype=torch.uint8, device=dev)
A = S.HASH_SHA256

# ---- (b) device-resident: messages forms against digest forms ----
fb = {"plain_digest": lambda: eng.ecdsa_verify_batch_device(N, p["pub"], p["dig"], p["r"], p["s"], dval.data_ptr(), stream=st),
      "plain_messages": lambda: eng.ecdsa_verify_messages_batch_device(N, p["pub"], A, p["msgs"], None, 32, p["r"], p["s"], dval.data_ptr(), stream=st),
      "bykey_digest": lambda: eng.ecdsa_verify_batch_bykey_device(ks, N, p["pub"], p["dig"], p["r"], p["s"], dval.data_ptr(), stream=st),
      "bykey_messages": lambda: eng.ecdsa_verify_messages_batch_bykey_device(ks, N, p["pub"], A, p["msgs"], None, 32, p["r"], p["s"], dval.data_ptr(), stream=st),
      "digest_kernel_sha256_32": lambda: eng.digest_batch_device(A, N, p["msgs"], None, 32, dout.data_ptr(), 32, stream=st)}
for k, f in fb.items():
    if k.startswith("digest"):
        continue
    dval.zero_()
    f()
    torch.cuda.synchronize()
    assert int(dval.sum().item()) == N, k
bms = {k: summary(m) for k, m in zip(fb, timed(list(fb.values()), events=True))}
emit(what="b_device_resident", n=N, keys=len(keys), layout="JOINT5", msg_len=32, alg="sha256", reps=args.reps, device=bms,
     plain_messages_minus_digest_ms=round(bms["plain_messages"]["ms"] - bms["plain_digest"]["ms"], 4),
     bykey_messages_minus_digest_ms=round(bms["bykey_messages"]["ms"] - bms["bykey_digest"]["ms"], 4))

# ---- (c) host to host from page-locked memory: synchronous, and four tickets in flight ----
h = {}
for k, x in (("pub", pub), ("dig", dig), ("r", r), ("s", s), ("msgs", msgs)):
    h[k] = S.pinned_array(x.shape)
    h[k][...] = x
hc = {"plain_digest": lambda: eng.ecdsa_verify_batch(h["pub"], h["dig"], h["r"], h["s"]),
      "plain_messages": lambda: eng.ecdsa_verify_messages_batch(h["pub"], h["msgs"], h["r"], h["s"], A),
      "bykey_digest": lambda: eng.ecdsa_verify_batch_bykey(ks, h["pub"], h["dig"], h["r"], h["s"]),
      "bykey_messages": lambda: eng.ecdsa_verify_messages_batch_bykey(ks, h["pub"], h["msgs"], h["r"], h["s"], A)}
for k, f in hc.items():
    assert int(f().sum()) == N, k
outs = [S.pinned_array((N,)) for _ in range(4)]


def tickets(submit):
    def g():
        ts = [submit(o) for o in outs]
        for t in ts:
            t.wait()
    return g


ht = {"plain_digest_4_tickets": tickets(lambda o: eng.ecdsa_verify_batch_submit(h["pub"], h["dig"], h["r"], h["s"], out=o)),
      "plain_messages_4_tickets": tickets(lambda o: eng.ecdsa_verify_messages_batch_submit(h["pub"], h["msgs"], h["r"], h["s"], A, out=o))}
for k, f in ht.items():
    f()
    assert all(int(o.sum()) == N for o in outs), k
cms = {k: summary(m) for k, m in zip(list(hc) + list(ht), timed(list(hc.values()) + list(ht.values()), events=False))}
for k in ht:
    cms[k + "_per_batch"] = {q: round(v / 4, 4) for q, v in cms[k].items()}
emit(what="c_host_to_host_pinned", n=N, keys=len(keys), layout="JOINT5", msg_len=32, alg="sha256", reps=args.reps, host=cms,
     host_hash_sha256_32_wall_ms=host_hash["sha256_32"]["wall"]["ms"])

# ---- (d) a small synchronous call ----
n1 = 1024
hd = {"digest_1024": lambda: eng.ecdsa_verify_batch(pub[:n1], dig[:n1], r[:n1], s[:n1]),
      "messages_1024": lambda: eng.ecdsa_verify_messages_batch(pub[:n1], msgs[:n1], r[:n1], s[:n1], A)}
for k, f in hd.items():
    assert int(f().sum()) == n1, k
t0 = time.perf_counter()
for i in range(n1):
    hashlib.sha256(msgs[i].tobytes()).digest()
one_thread_hash_ms = (time.perf_counter() - t0) * 1e3
dms = {k: summary(m) for k, m in zip(hd, timed(list(hd.values()) * 1, events=False))}
emit(what="d_small_call", n=n1, msg_len=32, alg="sha256", reps=args.reps, host=dms,
     messages_minus_digest_ms=round(dms["messages_1024"]["ms"] - dms["digest_1024"]["ms"], 4), hashlib_1024_one_thread_ms=round(one_thread_hash_ms, 4))
ks.close()
eng.close()
out_f.close()
