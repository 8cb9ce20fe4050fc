#!/usr/bin/env python3
"""Times the comb tables where BIP-340 calls and key sets use them, in ONE process with device-resident inputs and HIP events;
every figure is a median of REPS rounds, the variants alternated call by call.  2^20 signatures of 2^16 keys.

  --part ab       s2k_schnorr_verify_batch_device on the comb tables against the window tables of the same library
                  (s2k_ctx_set_keyed_ladder moved between calls), and the ECDSA pair the same way for scale
  --part keysets  s2k_ecdsa_verify_batch_keyset_device and s2k_schnorr_verify_batch_keyset_device over a set of the batch's keys
                  held as S2K_KEYSET_COMB, as S2K_KEYSET_CHUNKS and in the layout S2K_KEYSET_AUTO picks; each set's creation time
                  (wall clock, the call synchronises) and device bytes

One JSON line per result.  usage: schnorr_comb_time.py [--part ab|keysets|all] [--reps 9] [--quick]"""
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
ap.add_argument("--part", choices=("ab", "keysets", "all"), default="all")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--quick", action="store_true", help="2^16 signatures of 2^12 keys (a functional check of the tool)")
args = ap.parse_args()

eng = S.Engine(0, wait_tables=True)
lib, h = eng._lib, eng._h
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
N = 1 << (16 if args.quick else 20)
NKEYS = 1 << (12 if args.quick else 16)
LAYOUT_NAMES = {S.KEYSET_CHUNKS: "chunks", S.KEYSET_JOINT: "joint", S.KEYSET_JOINT5: "joint5", S.KEYSET_JOINT6: "joint6", S.KEYSET_COMB: "comb"}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fs):
    """medians (ms) of the callables in fs, alternated call by call"""
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
    return [float(np.median(m)) for m in ms], [[round(x, 4) for x in m] for m in ms]


pk, msgs, sig = synth_schnorr_batch(eng, N, NKEYS, seed=340)
dpk, dmsg, dsig = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pk, msgs, sig))
pub, dig, r, s = synth_batch(eng, N, NKEYS, seed=341)
dpub, ddig, dr, ds = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pub, dig, r, s))
dval = torch.zeros(N, dtype=torch.uint8, device=dev)


def all_valid(what):
    torch.cuda.synchronize()
    assert int(dval.sum().item()) == N, "%s did not accept the synthetic batch" % what
    dval.zero_()


if args.part in ("ab", "all"):
    def schnorr_on(ladder):
        def f():
            eng.set_keyed_ladder(ladder)
            assert lib.s2k_schnorr_verify_batch_device(h, N, dpk.data_ptr(), dmsg.data_ptr(), None, 32, dsig.data_ptr(), 0, dval.data_ptr(), st) == 0
            assert eng.last_keyed_ladder() == ladder
        return f

    def ecdsa_on(ladder):
        def f():
            eng.set_keyed_ladder(ladder)
            eng.ecdsa_verify_batch_device(N, dpub.data_ptr(), ddig.data_ptr(), dr.data_ptr(), ds.data_ptr(), dval.data_ptr(), stream=st)
            assert eng.last_keyed_ladder() == ladder
        return f

    for name, make in (("schnorr_verify_batch_device", schnorr_on), ("ecdsa_verify_batch_device", ecdsa_on)):
        for ladder in (S.LADDER_COMB, S.LADDER_WINDOW):
            make(ladder)()
            all_valid(name)
        (comb, window), raw = timed([make(S.LADDER_COMB), make(S.LADDER_WINDOW)])
        emit(what=name, sigs=N, keys=NKEYS, reps=args.reps, comb_ms=comb, window_ms=window, comb_over_window=comb / window,
             comb_ms_all=raw[0], window_ms_all=raw[1])
    eng.set_keyed_ladder(S.LADDER_COMB)

if args.part in ("keysets", "all"):
    def make_sets(keys):
        sets = {}
        for asked in (S.KEYSET_COMB, S.KEYSET_CHUNKS, S.KEYSET_AUTO):
            t0 = time.perf_counter()
            ks = eng.keyset_create(keys, asked)
            sets[asked] = (ks, time.perf_counter() - t0)
        return sets

    def report(what, sets, call):
        for ks, _ in sets.values():
            call(ks)()
            all_valid(what)
        order = list(sets)
        med, raw = timed([call(sets[a][0]) for a in order])
        for a, m, rw in zip(order, med, raw):
            ks, create_s = sets[a]
            emit(what=what, sigs=N, keys=len(ks), reps=args.reps, asked="auto" if a == S.KEYSET_AUTO else LAYOUT_NAMES[a],
                 layout=LAYOUT_NAMES[ks.layout()], ms=m, ms_all=rw, create_s=round(create_s, 4), device_bytes=ks.device_bytes(),
                 bytes_per_key=ks.device_bytes() / len(ks), geometry=list(S.keyset_geometry(ks.layout())))
        for ks, _ in sets.values():
            ks.close()

    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    dkidx = torch.from_numpy(inv.reshape(-1).astype(np.uint32).view(np.int32)).to(dev)
    report("ecdsa_verify_batch_keyset_device", make_sets(keys), lambda ks: lambda: eng.ecdsa_verify_batch_keyset_device(
        ks, N, dkidx.data_ptr(), ddig.data_ptr(), dr.data_ptr(), ds.data_ptr(), dval.data_ptr(), stream=st))
    xs, inv = np.unique(pk, axis=0, return_inverse=True)
    pts65, okd = eng.point_decode_batch(np.concatenate([np.full((len(xs), 1), 2, np.uint8), xs], axis=1), 33)
    assert bool(okd.all())
    xkeys = np.ascontiguousarray(pts65[:, 1:])
    odd = np.arange(len(xkeys)) % 2 == 1                     # every other key with the OTHER y: the sign flip of the ladder at work
    P_FIELD = 2**256 - 2**32 - 977
    xkeys[odd, 32:] = np.frombuffer(b"".join((P_FIELD - int.from_bytes(bytes(y), "big")).to_bytes(32, "big") for y in xkeys[odd, 32:]),
                                    np.uint8).reshape(-1, 32)
    dkidx = torch.from_numpy(inv.reshape(-1).astype(np.uint32).view(np.int32)).to(dev)
    report("schnorr_verify_batch_keyset_device", make_sets(xkeys), lambda ks: lambda: eng.schnorr_verify_batch_keyset_device(
        ks, N, dkidx.data_ptr(), dmsg.data_ptr(), 32, dsig.data_ptr(), dval.data_ptr(), st))
eng.close()
