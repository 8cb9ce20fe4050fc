#!/usr/bin/env python3
"""Times the Keccak digest kernel and the recovery calls that return addresses against plain recovery, in ONE process, the
variants alternated call by call; medians (with min and max) of REPS rounds after WARM warm-ups.

  a          k_digest_keccak alone (s2k_digest_batch_device, Keccak-256), 2^20 items of 32, 64, 136 and 250 bytes, with
             k_digest_messages (SHA-256) at the same lengths beside it; resident
  b          device-resident, 2^20 items: s2k_ecdsa_recover_batch_device (65-byte keys), s2k_ecdsa_recover_address_batch_device,
             the messages form at 110-byte messages, and k_keccak_address alone on the recovered keys
  c          host to host from page-locked memory: s2k_ecdsa_recover_batch plus the host hashing its keys, against
             s2k_ecdsa_recover_address_batch.  The host hash is hashlib.sha3_256 over 16 worker processes: a STAND-IN for
             Keccak-256 (hashlib has none; the same permutation count, another padding byte), labelled as that.  The workers
             are forked before the device is touched and read the keys from a shared, page-locked mapping.
  d          one call of 1024 items: recover against recover-address - the price of the second launch

  --part ab --parent-root DIR   `what: parent_ab`: the parent commit's package (a checkout of it with its library built, which
             lacks the new symbols and so needs its own binding) and this one in alternating child processes (this process
             never touches the device), s2k_ecdsa_recover_batch_device and s2k_digest_batch_device with SHA-256; appended to
             the file.  --part ab_child [--root DIR] is one such child.

usage: recover_address_time.py [--part main|ab|ab_child] [--reps 11] [--warm 3] [--n 1048576] [--keys 65536]
                               [--out profiles/r24_recover_address_time.jsonl]"""
import argparse
import hashlib
import json
import multiprocessing as mp
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="main", choices=["main", "ab", "ab_child"])
ap.add_argument("--parent-root", default="")
ap.add_argument("--root", default=ROOT)
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--reps", type=int, default=11)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=1 << 16)
ap.add_argument("--workers", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_recover_address_time.jsonl"))
args = ap.parse_args()
N, NKEYS, W = args.n, args.keys, args.workers
LENS = (32, 64, 136, 250)
MSG_LEN = 110
sys.path.insert(0, os.path.abspath(args.root))


def summary(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


# ---- the parent A/B: children only, this process holds no device ----
if args.part == "ab":
    assert os.path.isdir(os.path.join(args.parent_root, "secp256k1_voi_amd")), "--parent-root: a checkout of the parent commit, built"
    with open(args.out, "a") as f:
        for rnd in range(args.rounds):
            for name, root in (("parent", args.parent_root), ("new", ROOT)):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", "ab_child", "--root", os.path.abspath(root), "--reps", str(args.reps),
                                    "--warm", str(args.warm), "--n", str(N), "--keys", str(NKEYS)], capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.exit(f"child ({name}) failed with {p.returncode}: {p.stderr[-2000:]}")
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                rec["library"] = name
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
    sys.exit(0)

import secp256k1_voi_amd as S                                  # noqa: E402  (loads no device code yet)

rng = np.random.default_rng(2401)
MSGS = {L: rng.integers(0, 256, size=(N, L), dtype=np.uint8) for L in LENS + (MSG_LEN,)}
SHARED_KEYS = S.page_aligned_array((N, 65)) if args.part == "main" else None      # the workers inherit this mapping


def hash_keys(job):
    """addresses of the key records [lo, hi) of the shared mapping, with the stand-in hash"""
    lo, hi = job
    mv = memoryview(SHARED_KEYS).cast("B")
    return b"".join(hashlib.sha3_256(mv[i * 65 + 1:(i + 1) * 65]).digest()[12:] for i in range(lo, hi))


pool = mp.get_context("fork").Pool(W) if args.part == "main" else None            # forked from a process that holds no GPU
import torch                                                   # noqa: E402
from secp256k1_voi_amd.synth import synth_batch               # noqa: E402

eng = S.Engine(0, wait_tables=True)
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream


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


# the items: valid signatures, every recovery id 0 - half of them recover the signer's key and half another one, all of them a key
_, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, N, NKEYS, seed=2402))
rid = np.zeros(N, np.uint8)
d = {k: torch.from_numpy(x).to(dev) for k, x in (("dig", dig), ("r", r), ("s", s), ("rid", rid))}
p = {k: v.data_ptr() for k, v in d.items()}
dpub = torch.zeros(N * 65, dtype=torch.uint8, device=dev)
dok = torch.zeros(N, dtype=torch.uint8, device=dev)
f_recover = lambda: eng._check(eng._lib.s2k_ecdsa_recover_batch_device(eng._h, N, p["dig"], p["r"], p["s"], p["rid"], 0, dpub.data_ptr(), dok.data_ptr(), st))      # noqa: E731
dout = torch.zeros(N * 32, dtype=torch.uint8, device=dev)
dm32 = torch.from_numpy(MSGS[32]).to(dev)
f_sha256 = lambda: eng.digest_batch_device(S.HASH_SHA256, N, dm32.data_ptr(), None, 32, dout.data_ptr(), 32, stream=st)      # noqa: E731

if args.part == "ab_child":
    f_recover()
    torch.cuda.synchronize()
    assert int(dok.sum().item()) == N
    ms = timed([f_recover, f_sha256], events=True)
    print(json.dumps({"what": "parent_ab", "library": "?", "n": N, "reps": args.reps,
                      "device": {"recover_batch_device": summary(ms[0]), "digest_batch_device_sha256_32": summary(ms[1])}}), flush=True)
    eng.close()
    sys.exit(0)

out_f = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out_f.write(line + "\n")
    out_f.flush()


sys.path.insert(0, os.path.join(ROOT, "tests"))
import keccak_model as K                                       # noqa: E402  (spot checks)

# ---- (a) the digest kernels alone, device-resident ----
dmsgs = {L: torch.from_numpy(MSGS[L]).to(dev) for L in LENS}
names, fs = [], []
for name, alg in (("keccak256", S.HASH_KECCAK256), ("sha256", S.HASH_SHA256)):
    for L in LENS:
        f = (lambda alg=alg, L=L: eng.digest_batch_device(alg, N, dmsgs[L].data_ptr(), None, L, dout.data_ptr(), 32, stream=st))
        f()
        torch.cuda.synchronize()
        got = dout[:64 * 32].cpu().numpy().reshape(64, 32)
        ref = K.keccak256 if name == "keccak256" else (lambda m: hashlib.sha256(m).digest())
        assert all(bytes(got[i]) == ref(bytes(MSGS[L][i])) for i in range(64)), (name, L)
        names.append(f"{name}_{L}")
        fs.append(f)
ams = {k: summary(m) for k, m in zip(names, timed(fs, events=True))}
emit(what="a_digest_kernel", n=N, reps=args.reps, device=ams)

# ---- (b) device-resident: recovery, recovery to addresses, the same from messages, the address kernel alone ----
daddr = torch.zeros(N * 20, dtype=torch.uint8, device=dev)
dm = torch.from_numpy(MSGS[MSG_LEN]).to(dev)
fb = {"recover": f_recover,
      "recover_address": lambda: eng.ecdsa_recover_address_batch_device(N, p["dig"], p["r"], p["s"], p["rid"], daddr.data_ptr(), dok.data_ptr(), stream=st),
      "recover_address_messages": lambda: eng.ecdsa_recover_address_messages_batch_device(N, S.HASH_KECCAK256, dm.data_ptr(), None, MSG_LEN, p["r"], p["s"],
                                                                                          p["rid"], daddr.data_ptr(), dok.data_ptr(), stream=st),
      "keccak_address_kernel": lambda: eng.keccak_address_batch_device(N, dpub.data_ptr(), dok.data_ptr(), daddr.data_ptr(), stream=st),
      "digest_kernel_keccak256_110": lambda: eng.digest_batch_device(S.HASH_KECCAK256, N, dm.data_ptr(), None, MSG_LEN, dout.data_ptr(), 32, stream=st)}
fb["recover"]()
fb["recover_address"]()
torch.cuda.synchronize()
assert int(dok.sum().item()) == N
keys_h, addr_h = dpub[:64 * 65].cpu().numpy().reshape(64, 65), daddr[:64 * 20].cpu().numpy().reshape(64, 20)
assert all(bytes(addr_h[i]) == K.address(bytes(keys_h[i][1:])) for i in range(64))
bms = {k: summary(m) for k, m in zip(fb, timed(list(fb.values()), events=True))}
emit(what="b_device_resident", n=N, msg_len=MSG_LEN, alg="keccak256", reps=args.reps, device=bms,
     recover_address_minus_recover_ms=round(bms["recover_address"]["ms"] - bms["recover"]["ms"], 4),
     messages_minus_recover_ms=round(bms["recover_address_messages"]["ms"] - bms["recover"]["ms"], 4),
     keccak_kernels_share_of_messages_call=round((bms["keccak_address_kernel"]["ms"] + bms["digest_kernel_keccak256_110"]["ms"]) / bms["recover_address_messages"]["ms"], 4))

# ---- (c) host to host from page-locked memory ----
S.host_register(SHARED_KEYS)
h = {}
for k, x in (("dig", dig), ("r", r), ("s", s), ("rid", rid)):
    h[k] = S.pinned_array(x.shape)
    h[k][...] = x
h_ok, h_addr = S.pinned_array((N,)), S.pinned_array((N, 20))
per = (N + W - 1) // W
jobs = [(lo, min(N, lo + per)) for lo in range(0, N, per)]
hp = {k: v.ctypes.data for k, v in h.items()}
host_hash_ms = []


def recover_then_host_hash():
    eng._check(eng._lib.s2k_ecdsa_recover_batch(eng._h, N, hp["dig"], hp["r"], hp["s"], hp["rid"], 0, SHARED_KEYS.ctypes.data, h_ok.ctypes.data))
    t0 = time.perf_counter()
    blob = b"".join(pool.map(hash_keys, jobs))
    host_hash_ms.append((time.perf_counter() - t0) * 1e3)
    return blob


def recover_address():
    eng._check(eng._lib.s2k_ecdsa_recover_address_batch(eng._h, N, hp["dig"], hp["r"], hp["s"], hp["rid"], 0, h_addr.ctypes.data, h_ok.ctypes.data))


blob = recover_then_host_hash()
assert len(blob) == 20 * N and blob[:20] == hashlib.sha3_256(bytes(SHARED_KEYS[0][1:])).digest()[12:]
recover_address()
assert int(h_ok.sum()) == N and bytes(h_addr[5]) == K.address(bytes(SHARED_KEYS[5][1:]))
host_hash_ms.clear()
cms = {k: summary(m) for k, m in zip(("recover_plus_host_hash", "recover_address"), timed([recover_then_host_hash, recover_address], events=False))}
cms["host_hash_alone"] = summary(host_hash_ms[args.warm:])
emit(what="c_host_to_host_pinned", n=N, reps=args.reps, host=cms, host_hash="hashlib.sha3_256 as a stand-in for Keccak-256 (same permutation count)",
     workers=W, cpus=os.cpu_count(), saved_ms=round(cms["recover_plus_host_hash"]["ms"] - cms["recover_address"]["ms"], 4))
S.host_unregister(SHARED_KEYS)
pool.close()
pool.join()

# ---- (d) one call of 1024 items ----
n1 = 1024
hd = {"recover_1024": lambda: eng.ecdsa_recover_batch(dig[:n1], r[:n1], s[:n1], rid[:n1]),
      "recover_address_1024": lambda: eng.ecdsa_recover_address_batch(dig[:n1], r[:n1], s[:n1], rid[:n1])}
pk, _ = hd["recover_1024"]()
ad, _ = hd["recover_address_1024"]()
assert np.array_equal(ad, eng.keccak_address_batch(pk))
dms = {k: summary(m) for k, m in zip(hd, timed(list(hd.values()), events=False))}
emit(what="d_small_call", n=n1, reps=args.reps, host=dms, second_launch_ms=round(dms["recover_address_1024"]["ms"] - dms["recover_1024"]["ms"], 4))
eng.close()
out_f.close()
