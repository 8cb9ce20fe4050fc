"""Sanitizer run of the property s2k_keyset_append rests on (csrc/keyset_index.h, plain-memory policy): an index that is built
over the first part of a key list and then handed the rest in ranges answers every lookup - 64, 32, 33 bytes and x-only among
the valid keys - as a brute-force scan of the live keys does, after every range: duplicates, Q / -Q pairs and invalid entries
on both sides of the boundary, a table one slot short of full.  A stand-alone program (tests/c/keyset_index_append_main.cpp)
built for the host with AddressSanitizer + UndefinedBehaviorSanitizer; no device code, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest


def test_keyset_index_append_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "keyset_index_append_san")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "secp256k1_voi_amd", "csrc"),
                           os.path.join(root, "tests", "c", "keyset_index_append_main.cpp"), "-o", exe])
    p = subprocess.run([exe, "0x5ec9", "1", "0xfeedfacecafebeef", "0x0123456789abcdef"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok 4 seeds"), p.stdout + p.stderr[-2000:]
