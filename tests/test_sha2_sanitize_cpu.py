"""Sanitizer run of the hash cores of the message digests (csrc/sha2.h: SHA-256, double SHA-256 and SHA-512 take a
caller-supplied length), in their host build: a stand-alone program, built with AddressSanitizer +
UndefinedBehaviorSanitizer and run on the CPU.  It prints digests; they are compared with hashlib here.  No device code is
involved and nothing is loaded into Python."""
import hashlib
import os
import shutil
import subprocess

import pytest

# FIPS 180-4 example messages (the program embeds the same four): "abc", empty, 448 bits, 896 bits
FIPS = [b"abc", b"", b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
        b"abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"]
# ... and two of their digests as the standard prints them, so that hashlib is not the only witness
FIPS_KNOWN = {(0, 0): "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
              (2, 0): "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1",
              (0, 2): "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a"
                      "2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
              (3, 2): "8e959b75dae313da8cf4f72814fc143f8f7779c6eb9f7fa17299aeadb6889018"
                      "501d289e4900f7e4331b99dec4b5433ac7d329eeb6dd26545e96e55b874be909"}


def expected(msg):
    return [hashlib.sha256(msg).hexdigest(), hashlib.sha256(hashlib.sha256(msg).digest()).hexdigest(), hashlib.sha512(msg).hexdigest()]


def test_sha2_host_build_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "sha2_san")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "secp256k1_voi_amd", "csrc"),
                           os.path.join(root, "tests", "c", "sha2_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.split("\n")
    assert lines[-2:] == ["done", ""] and len(lines) == 4 + 301 + 2
    for k, msg in enumerate(FIPS):
        kind, tag, *got = lines[k].split(" ")
        assert (kind, int(tag)) == ("fips", k) and got == expected(msg), lines[k]
        for alg in range(3):
            if (k, alg) in FIPS_KNOWN:
                assert got[alg] == FIPS_KNOWN[(k, alg)]
    for n in range(301):
        msg = bytes((131 * i + 7 * n + 1) & 0xff for i in range(n))
        kind, tag, *got = lines[4 + n].split(" ")
        assert (kind, int(tag)) == ("len", n) and got == expected(msg), lines[4 + n]
