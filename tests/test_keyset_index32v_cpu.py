"""Sanitizer run of the valid-only x-only probe of a key set's index (csrc/keyset_index.h: ksi_lookup32v with the plain-memory
policy), the lookup of s2k_schnorr_verify_batch_keyset_bykey: a stand-alone program (tests/c/keyset_index32v_main.cpp), built
for the host with AddressSanitizer + UndefinedBehaviorSanitizer and run on the CPU, that compares every lookup with a brute-force
scan of the key list.  No device code is involved and nothing is loaded into Python.

The set is made here, of real points (multiples of the generator from pyref's affine addition - the engine is not used) and of
entries that are no public keys; which entries are valid is computed from the coordinates (canonical, on the curve), as the
library does when it builds a set.  About 1000 entries: plain keys, Q / -Q pairs in both orders, duplicates, X held only by an
entry off the curve, an entry off the curve at a lower index than the real point with its X and the reverse order, entries
with X >= p; indexed with the automatic geometry and nearly full (1024 slots), under a fixed hash seed and three others."""
import os
import random
import shutil
import subprocess

import pytest

import pyref as R


def _is_key(k):
    x, y = int.from_bytes(k[:32], "big"), int.from_bytes(k[32:], "big")
    return x < R.P and y < R.P and R.on_curve((x, y))


def make_set():
    rng = random.Random(3201)
    pts, p = [], None
    for _ in range(960):
        p = R.add(p, R.G)
        pts.append(p)
    rng.shuffle(pts)                                             # (X of k G in no order)
    key = lambda pt: R.b32(pt[0]) + R.b32(pt[1])
    off = lambda pt: R.b32(pt[0]) + R.b32(pt[1] ^ 1)             # the same X, Y one off: not on the curve
    plain, pairs, only_bad, bad_first, bad_last = pts[:900], pts[900:920], pts[920:930], pts[930:940], pts[940:950]
    middle = [key(q) for q in plain]
    for j, q in enumerate(pairs):                                # Q and -Q, in either order
        middle += [key(q), key(R.neg(q))] if j % 2 else [key(R.neg(q)), key(q)]
    middle += [off(q) for q in only_bad]                         # X held only by an invalid entry
    middle += [R.b32(R.P + 5) + R.b32(pts[950][1]), b"\xff" * 64]   # X >= p
    rng.shuffle(middle)
    entries = [off(q) for q in bad_first] + [key(q) for q in bad_last] + middle + \
              [key(q if j % 2 else R.neg(q)) for j, q in enumerate(bad_first)] + [off(q) for q in bad_last]
    for _ in range(30):                                          # duplicates of valid and of invalid entries
        entries.insert(rng.randrange(len(entries) + 1), entries[rng.randrange(len(entries))])
    valid = [1 if _is_key(k) else 0 for k in entries]
    # what the list was built to hold is still there after the duplicates went in
    first_any, first_valid = {}, {}
    for i, (k, v) in enumerate(zip(entries, valid)):
        first_any.setdefault(k[:32], i)
        if v:
            first_valid.setdefault(k[:32], i)
    xs = lambda group: [R.b32(q[0]) for q in group]
    assert all(x not in first_valid for x in xs(only_bad))
    assert sum(first_any[x] < first_valid[x] for x in xs(bad_first)) >= 5          # the invalid entry first
    assert sum(first_any[x] == first_valid[x] for x in xs(bad_last)) >= 5          # the valid entry first
    assert R.b32(R.P + 5) in first_any and R.b32(R.P + 5) not in first_valid
    assert len(entries) == 1022 and 940 < sum(valid) < 1000 and len(set(entries)) == 992
    return entries, valid


def test_new_calls_refuse_without_a_device_and_are_bound():
    """the fused BIP-340 call and the ticket forms: the refusals that precede every HIP call, and the binding"""
    import ctypes as C
    import numpy as np
    import secp256k1_voi_amd as S
    lib = S.load_library()
    ERR_ARG = -3
    buf = np.full(64, 0xAB, dtype=np.uint8)
    p = buf.ctypes.data
    t = C.c_uint64(7)
    assert lib.s2k_schnorr_verify_batch_keyset_bykey(None, None, 1, p, p, None, 32, p, 0, p) == ERR_ARG
    assert lib.s2k_schnorr_verify_batch_keyset_bykey_device(None, None, 0, None, None, None, 0, None, 0, None, None) == ERR_ARG
    assert lib.s2k_schnorr_verify_batch_keyset_bykey_submit(None, None, 1, p, p, None, 32, p, 0, p, C.byref(t)) == ERR_ARG
    assert lib.s2k_ecdsa_verify_batch_keyset_bykey_submit(None, None, 1, p, p, p, p, 0, p, C.byref(t)) == ERR_ARG
    assert (buf == 0xAB).all() and t.value == 7
    for name in ("s2k_schnorr_verify_batch_keyset_bykey", "s2k_schnorr_verify_batch_keyset_bykey_device",
                 "s2k_schnorr_verify_batch_keyset_bykey_submit", "s2k_ecdsa_verify_batch_keyset_bykey_submit"):
        assert name in S.EXPORTED_SYMBOLS and getattr(lib, name).argtypes, name
    for method in ("schnorr_verify_batch_bykey", "schnorr_verify_batch_bykey_device", "schnorr_verify_batch_bykey_submit",
                   "ecdsa_verify_batch_bykey_submit"):
        assert callable(getattr(S.Engine, method)), method


def test_keyset_index32v_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    entries, valid = make_set()
    set_file = str(tmp_path / "set.bin")
    with open(set_file, "wb") as f:
        f.write(len(entries).to_bytes(4, "little") + b"".join(entries) + bytes(valid))
    exe = str(tmp_path / "keyset_index32v_san")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "secp256k1_voi_amd", "csrc"),
                           os.path.join(root, "tests", "c", "keyset_index32v_main.cpp"), "-o", exe])
    p = subprocess.run([exe, set_file, "0x5ec9", "1", "0xfeedfacecafebeef", "0x0123456789abcdef"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok 4 seeds, 1022 keys"), p.stdout + p.stderr[-2000:]
