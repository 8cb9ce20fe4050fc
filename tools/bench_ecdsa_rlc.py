#!/usr/bin/env python3
"""Whole-batch verification of recoverable ECDSA signatures on one GPU: time of s2k_ecdsa_batch_verify_rlc_device beside the
two per-signature calls it competes with, on the same inputs.

    timeout 900 python tools/bench_ecdsa_rlc.py [--batch-log2 20] [--reps 20] [--warmup 3] [--out FILE]

2^batch_log2 valid low-s signatures from synth_batch, once under 2^16 keys and once with every key distinct, inputs resident
on the device, warm.  The recovery id of every item is derived by running the recovery call with id 0 and with id 1 and
keeping the one whose key is the item's; before anything is timed every item must have got one, and the first 256 are
compared with the oracle.  Per key count the three calls are timed ALTERNATELY, repetition by repetition, in one process:
    rlc      s2k_ecdsa_batch_verify_rlc_device (synchronises its stream for the verdict)
    keyed    (a) the resident s2k_ecdsa_verify_batch_device step of bench.py
    recover  (b) s2k_ecdsa_recover_batch_device
and the median, the fastest and the slowest of --reps repetitions of each are reported, with rlc's median over (a)'s median
and whether rlc's median is below (a)'s FASTEST repetition.  Prints ONE JSON line; --out also writes it to a file.
One process; run it under `timeout`."""
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


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_ecdsa_rlc.py: no GPU (there is no CPU fallback, and a CPU time would say nothing)", file=sys.stderr)
        return 2
    import oracle
    from secp256k1_voi_amd.synth import synth_batch
    oracle.build()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    n = 1 << a.batch_log2
    eng = S.Engine(0)
    eng.gt_wait()
    st = torch.cuda.current_stream().cuda_stream
    seed = bytes(range(32))
    line = {"tool": "bench_ecdsa_rlc", "n": n, "device": torch.cuda.get_device_name(0),
            "build": S.load_library().s2k_build_config().decode()}
    for label, nkeys in (("keys_2p16", min(n, 1 << 16)), ("keys_distinct", n)):
        pub, digest, r_, s_ = synth_batch(eng, n, nkeys, seed=0x5EC9 + nkeys)
        rid = np.full(n, 255, dtype=np.uint8)
        for v in (0, 1):
            rec, ok = eng.ecdsa_recover_batch(digest, r_, s_, np.full(n, v, dtype=np.uint8))
            hit = (ok == 1) & (rec[:, 0] == 4) & (rec[:, 1:] == pub).all(axis=1)
            rid[hit] = v
        assert (rid <= 1).all(), "an item has no recovery id under which its key comes back"
        for i in range(min(256, n)):
            assert oracle.ecdsa_recover(bytes(digest[i]), bytes(r_[i]), bytes(s_[i]), int(rid[i])) == b"\x04" + bytes(pub[i]), i
        d_pub, d_dig, d_r, d_s, d_rid = (torch.from_numpy(x).to(dev) for x in (pub, digest, r_, s_, rid))
        d_valid = torch.zeros(n, dtype=torch.uint8, device=dev)
        d_rec = torch.zeros(n * 65, dtype=torch.uint8, device=dev)
        d_ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        verdicts = []

        def rlc():
            verdicts.append(eng.ecdsa_batch_verify_rlc_device(n, d_pub.data_ptr(), d_dig.data_ptr(), d_r.data_ptr(), d_s.data_ptr(),
                                                              d_rid.data_ptr(), seed, 0, st))

        def keyed():
            eng.ecdsa_verify_batch_device(n, d_pub.data_ptr(), d_dig.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_valid.data_ptr(), 0, st)

        def recover():
            eng._check(eng._lib.s2k_ecdsa_recover_batch_device(eng._h, n, d_dig.data_ptr(), d_r.data_ptr(), d_s.data_ptr(), d_rid.data_ptr(),
                                                               0, d_rec.data_ptr(), d_ok.data_ptr(), st))
        calls = (("rlc", rlc), ("keyed", keyed), ("recover", recover))
        for _ in range(a.warmup):
            for _, fn in calls:
                fn()
                torch.cuda.synchronize()
        assert all(verdicts), "the whole-batch call rejected a good batch"
        assert int(d_valid.sum().item()) == n and int(d_ok.sum().item()) == n, "synthetic batch did not verify"
        ms = {name: [] for name, _ in calls}
        for _ in range(a.reps):
            for name, fn in calls:                       # alternately: the three share the box's state of the moment
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
        assert all(verdicts)
        res = {name: summary(v) for name, v in ms.items()}
        res["n_keys"] = nkeys
        res["rlc_over_keyed"] = res["rlc"]["median_ms"] / res["keyed"]["median_ms"]
        res["rlc_over_recover"] = res["rlc"]["median_ms"] / res["recover"]["median_ms"]
        res["rlc_median_below_keyed_fastest"] = res["rlc"]["median_ms"] < res["keyed"]["min_ms"]
        line[label] = res
        del d_pub, d_dig, d_r, d_s, d_rid, d_valid, d_rec, d_ok
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
