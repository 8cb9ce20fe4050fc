#!/usr/bin/env python3
"""Hashing to the curve on one GPU: time of s2k_hash_to_curve_batch_device for both suites.

    timeout 600 python tools/bench_h2c.py [--batch-log2 20] [--msg-len 32] [--reps 20] [--warmup 3] [--no-ecdsa] [--out FILE]

2^batch_log2 messages of msg_len bytes (fixed-length form), the 49-byte tag of the RFC's RO suite, inputs and outputs
resident on the device, warm.  The call synchronises its stream (it reads back its status word), so the host clock around
a call measures launch to completion; the median over --reps calls is reported, with the fastest and the slowest.  For a
yardstick of the same session on the same box, the resident keyed ECDSA step of bench.py (2^batch_log2 signatures of 2^16
keys through s2k_ecdsa_verify_batch_device, wide generator tables) is timed the same way unless --no-ecdsa.  Before
anything is timed, the first 256 records of each suite are compared with tests/h2c_model.py.  Prints ONE JSON line; --out
also writes it to a file.  One process; run it under `timeout`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp256k1_voi_amd as S

DST = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"


def timed(fn, sync, reps, warmup):
    for _ in range(warmup):
        fn()
    sync()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-log2", type=int, default=20)
    ap.add_argument("--msg-len", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-ecdsa", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_h2c.py: no GPU (there is no CPU fallback, and a CPU time would say nothing)", file=sys.stderr)
        return 2
    import h2c_model as M
    import pyref
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n = 1 << a.batch_log2
    eng = S.Engine(0)
    rng = np.random.default_rng(0x4832C)
    msgs = rng.integers(0, 256, size=(n, a.msg_len), dtype=np.uint8)
    d_msgs = torch.from_numpy(msgs).to(dev)
    d_out = torch.zeros(n * 65, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    total = n * a.msg_len
    line = {"tool": "bench_h2c", "n": n, "msg_len": a.msg_len, "dst_len": len(DST), "device": torch.cuda.get_device_name(0),
            "build": S.load_library().s2k_build_config().decode()}
    for name, suite, model in (("hash_to_curve_ro", S.H2C_SSWU_RO, M.hash_to_curve), ("encode_to_curve_nu", S.H2C_SSWU_NU, M.encode_to_curve)):
        def call():
            eng.hash_to_curve_device(suite, n, DST, d_msgs.data_ptr(), None, a.msg_len, total, d_out.data_ptr(), st)
        d_out.zero_()
        call()
        k = min(256, n)
        head = d_out[:k * 65].cpu().numpy().reshape(k, 65)
        tail = d_out[(n - 1) * 65:].cpu().numpy()
        for i in range(k):
            assert head[i].tobytes() == pyref.enc65(model(msgs[i].tobytes(), DST)[0]), (name, i)
        assert tail.tobytes() == pyref.enc65(model(msgs[n - 1].tobytes(), DST)[0]), (name, n - 1)
        r = timed(call, torch.cuda.synchronize, a.reps, a.warmup)
        r["messages_per_s"] = n / (r["median_ms"] * 1e-3)
        line[name] = r
    if not a.no_ecdsa:
        from secp256k1_voi_amd.synth import synth_batch
        eng.gt_wait()
        pub, digest, r_, s_ = synth_batch(eng, n, min(n, 1 << 16), seed=0x5EC9)
        d_pub, d_dig, d_r, d_s = (torch.from_numpy(x).to(dev) for x in (pub, digest, r_, s_))
        d_valid = torch.zeros(n, dtype=torch.uint8, device=dev)

        def step():
            eng.ecdsa_verify_batch_device(n, d_pub.data_ptr(), d_dig.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_valid.data_ptr(), 0, st)
        step()
        torch.cuda.synchronize()
        assert int(d_valid.sum().item()) == n, "synthetic batch did not verify"
        r = timed(step, torch.cuda.synchronize, a.reps, a.warmup)
        r["verifications_per_s"] = n / (r["median_ms"] * 1e-3)
        line["ecdsa_keyed_resident"] = r
        line["ro_over_ecdsa"] = line["hash_to_curve_ro"]["median_ms"] / r["median_ms"]
    eng.close()
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
