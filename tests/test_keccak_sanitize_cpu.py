"""Sanitizer run of the Keccak cores (csrc/keccak.h: Keccak-256 and SHA3-256 take a caller-supplied length; keccak256_64 is
the fixed block of the addresses), in their host build: a stand-alone program, built with AddressSanitizer +
UndefinedBehaviorSanitizer and run on the CPU.  It prints digests; they are compared here with hashlib (SHA3-256) and with
tests/keccak_model.py (Keccak-256).  No device code is involved and nothing is loaded into Python."""
import hashlib
import os
import shutil
import subprocess

import pytest

import keccak_model as K
import pyref as R

VEC = [b"", b"abc", R.b32(R.GX) + R.b32(R.GY)]
VEC_KNOWN = {0: "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470",
             1: "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"}


def expected(msg):
    return [K.keccak256(msg).hex(), hashlib.sha3_256(msg).hexdigest()]


def test_keccak_host_build_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "keccak_san")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "secp256k1_voi_amd", "csrc"),
                           os.path.join(root, "tests", "c", "keccak_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.split("\n")
    assert lines[-2:] == ["done", ""] and len(lines) == 3 + 301 + 16 + 2
    for k, msg in enumerate(VEC):
        kind, tag, *got = lines[k].split(" ")
        assert (kind, int(tag)) == ("vec", k) and got == expected(msg), lines[k]
        if k in VEC_KNOWN:
            assert got[0] == VEC_KNOWN[k]
    assert lines[2].split(" ")[2][24:] == "7e5f4552091a69125d5dfcb7b8c2659029395bdf"      # the address of the key of secret 1
    for n in range(301):
        msg = bytes((131 * i + 7 * n + 1) & 0xff for i in range(n))
        kind, tag, *got = lines[3 + n].split(" ")
        assert (kind, int(tag)) == ("len", n) and got == expected(msg), lines[3 + n]
        assert got[1] == K.sha3_256(msg).hex()
    for t in range(16):
        xy = bytes(0 if t == 0 else (0xff if t == 1 else (29 * i + 83 * t + (i >> 3) * t) & 0xff) for i in range(64))
        kind, tag, one, gen = lines[304 + t].split(" ")
        assert (kind, int(tag)) == ("xy", t) and one == gen == K.keccak256(xy).hex(), lines[304 + t]
