#!/usr/bin/env python3
"""Times ECDSA verification of ENCODED batches (SEC1 keys, DER signatures) against a long-lived key set, in ONE process, the
variants alternated call by call; medians (with min and max) of REPS rounds after WARM warm-ups.  2^20 signatures over 2^16
keys, a JOINT5 and a COMB set, each with an index.  Host to host (wall clock) throughout: the inputs are page-locked
(blob, offsets) pairs, so no Python work is inside the clock.

  a    the plain ecdsa_verify_encoded_batch on compressed keys + DER (a square root per key in the parse kernel)
  a65  the same on uncompressed keys: a - a65 is what decompression costs there
  raw  the plain ecdsa_verify_batch on the pre-parsed arrays: a65 - raw is what parsing costs there
  c33  ecdsa_verify_encoded_batch_keyset, every key in the set, compressed keys (no square root at all); c65: uncompressed
  d33  the same with 1/16 of the signatures under keys outside the set (the decompression list, the general ladder); d65
  f    ecdsa_verify_batch_bykey on the pre-parsed arrays: the floor that leaves only parsing in c - f

Each as the synchronous call and as four tickets in flight (ms per batch = the time from the first submit to the last wait,
by four); `f` has no ticket form.  One JSON line per layout.  --variants selects a subset (a kernel-trace run: a,c33,d33
with --no-tickets gives every launch of a parse kernel one case).

usage: encoded_keyset_time.py [--reps 9] [--warm 2] [--n 1048576] [--keys 65536] [--layouts JOINT5,COMB] [--variants ...]
                              [--no-tickets] [--out profiles/r16_encoded_keyset_time.jsonl]"""
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

ALL = ["a", "a65", "raw", "c33", "c65", "d33", "d65", "f"]
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--keys", type=int, default=1 << 16)
ap.add_argument("--layouts", default="JOINT5,COMB")
ap.add_argument("--variants", default=",".join(ALL))
ap.add_argument("--no-tickets", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_encoded_keyset_time.jsonl"))
args = ap.parse_args()
N, NKEYS = args.n, args.keys
want = [v for v in ALL if v in args.variants.split(",")]

assert torch.cuda.is_available()
torch.cuda.init()
eng = S.Engine(0, wait_tables=True)
out_f = open(args.out, "w")


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    out_f.write(line + "\n")
    out_f.flush()


def pinned(a):
    p = S.pinned_array(a.shape, a.dtype)
    p[...] = a
    return p


def fixed(rows):
    """(blob, offsets) of n strings of one length"""
    n, w = rows.shape
    return pinned(np.ascontiguousarray(rows).reshape(-1)), pinned(np.arange(n + 1, dtype=np.uint64) * np.uint64(w))


def der_blob(r, s):
    """strict DER of every (r, s): (blob, offsets), built row by row (minimal integers: leading zeros stripped, a zero byte in
    front of a set top bit)"""
    def integer(x):
        x = bytes(x).lstrip(b"\0") or b"\0"
        if x[0] & 0x80:
            x = b"\0" + x
        return b"\x02" + bytes([len(x)]) + x
    items = []
    for i in range(len(r)):
        body = integer(r[i]) + integer(s[i])
        items.append(b"\x30" + bytes([len(body)]) + body)
    offs = np.zeros(len(items) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    return pinned(np.frombuffer(b"".join(items), np.uint8)), pinned(offs)


def encodings(pub, dig, r, s):
    c = np.empty((len(pub), 33), np.uint8)
    c[:, 0] = 2 + (pub[:, 63] & 1)
    c[:, 1:] = pub[:, :32]
    u = np.concatenate([np.full((len(pub), 1), 4, np.uint8), pub], axis=1)
    return dict(k33=fixed(c), k65=fixed(u), dig=fixed(dig), der=der_blob(r, s), raw=tuple(pinned(x) for x in (pub, dig, r, s)))


def summary(ms):
    return {"ms": round(float(np.median(ms)), 4), "min": round(float(min(ms)), 4), "max": round(float(max(ms)), 4)}


def timed(fs):
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


# the batch: N valid signatures of NKEYS keys; its variant with every 16th signature under a key the set does not hold
pub, dig, r, s = (np.ascontiguousarray(x) for x in synth_batch(eng, N, NKEYS, seed=1601))
keys = np.unique(pub, axis=0)
n_out = len(pub[::16])
opub, odig, orr, oss = (np.ascontiguousarray(x) for x in synth_batch(eng, n_out, max(NKEYS // 16, 1), seed=1602))
pub2, dig2, r2, s2 = pub.copy(), dig.copy(), r.copy(), s.copy()
pub2[::16], dig2[::16], r2[::16], s2[::16] = opub, odig, orr, oss
E1, E2 = encodings(pub, dig, r, s), encodings(pub2, dig2, r2, s2)

for name in args.layouts.split(","):
    ks = eng.keyset_create(keys, getattr(S, "KEYSET_" + name))
    ks.index_create()
    sync = {
        "a": lambda: eng.ecdsa_verify_encoded_batch(E1["k33"], E1["dig"], E1["der"]),
        "a65": lambda: eng.ecdsa_verify_encoded_batch(E1["k65"], E1["dig"], E1["der"]),
        "raw": lambda: eng.ecdsa_verify_batch(*E1["raw"]),
        "c33": lambda: eng.ecdsa_verify_encoded_batch_keyset(ks, E1["k33"], E1["dig"], E1["der"]),
        "c65": lambda: eng.ecdsa_verify_encoded_batch_keyset(ks, E1["k65"], E1["dig"], E1["der"]),
        "d33": lambda: eng.ecdsa_verify_encoded_batch_keyset(ks, E2["k33"], E2["dig"], E2["der"]),
        "d65": lambda: eng.ecdsa_verify_encoded_batch_keyset(ks, E2["k65"], E2["dig"], E2["der"]),
        "f": lambda: eng.ecdsa_verify_batch_bykey(ks, *E1["raw"]),
    }
    submit = {
        "a": lambda: eng.ecdsa_verify_encoded_batch_submit(E1["k33"], E1["dig"], E1["der"]),
        "a65": lambda: eng.ecdsa_verify_encoded_batch_submit(E1["k65"], E1["dig"], E1["der"]),
        "raw": lambda: eng.ecdsa_verify_batch_submit(*E1["raw"]),
        "c33": lambda: eng.ecdsa_verify_encoded_batch_keyset_submit(ks, E1["k33"], E1["dig"], E1["der"]),
        "c65": lambda: eng.ecdsa_verify_encoded_batch_keyset_submit(ks, E1["k65"], E1["dig"], E1["der"]),
        "d33": lambda: eng.ecdsa_verify_encoded_batch_keyset_submit(ks, E2["k33"], E2["dig"], E2["der"]),
        "d65": lambda: eng.ecdsa_verify_encoded_batch_keyset_submit(ks, E2["k65"], E2["dig"], E2["der"]),
    }
    # every variant accepts the synthetic batch; hits, misses and square roots as planned
    stats = {}
    for k in want:
        assert int(sync[k]().sum()) == N, k
        if k[0] in "cd":
            stats[k] = dict(eng.last_encoded_keyset_stats(), **eng.key_grouping_stats())
    for k, st in stats.items():
        out = n_out if k[0] == "d" else 0
        assert st["hits33" if k.endswith("33") else "hits65"] == N - out and st["roots"] == (out if k.endswith("33") else 0), (k, st)

    def four(f):
        def g():
            ts = [f() for _ in range(4)]
            for t in ts:
                t.wait()
        return g
    H = {k: summary(m) for k, m in zip(want, timed([sync[k] for k in want]))}
    T = {}
    if not args.no_tickets:
        tw = [k for k in want if k in submit]
        T = {k: summary([x / 4 for x in m]) for k, m in zip(tw, timed([four(submit[k]) for k in tw]))}
    derived = {}
    if all(k in H for k in ("a", "a65", "raw", "c33", "f")):
        derived = dict(decompression_ms=round(H["a"]["ms"] - H["a65"]["ms"], 4), plain_parse_ms=round(H["a65"]["ms"] - H["raw"]["ms"], 4),
                       keyset_parse_ms=round(H["c33"]["ms"] - H["f"]["ms"], 4), c33_over_a=round(H["c33"]["ms"] / H["a"]["ms"], 4))
    emit(what="encoded_keyset", layout=name, n=N, keys=len(keys), outside=n_out, reps=args.reps, bytes_per_signature=dict(
        k33=round((E1["k33"][0].size + E1["dig"][0].size + E1["der"][0].size + 24 * N) / N, 1),
        k65=round((E1["k65"][0].size + E1["dig"][0].size + E1["der"][0].size + 24 * N) / N, 1), raw=160),
        sync=H, tickets=T, stats=stats, **derived)
    ks.close()
eng.close()
out_f.close()
