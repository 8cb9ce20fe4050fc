"""Sanitizer run of the compressed-key probe of a key set's index (csrc/keyset_index.h: ksi_lookup33 with the plain-memory
policy): a stand-alone program, built for the host with AddressSanitizer + UndefinedBehaviorSanitizer and run on the CPU, that
compares every lookup with a brute-force scan of the key list - pairs Q / -Q, duplicates, keys flagged invalid that share X
and parity with a valid key at a lower and at a higher index, invalid keys alone on their X, a table with one empty slot;
both prefixes, the prefixes 00 / 04 / 05, and X one bit away from a stored X; under a fixed hash seed and three others.  No
device code is involved and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest


def test_keyset_index33_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "keyset_index33_san")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "secp256k1_voi_amd", "csrc"),
                           os.path.join(root, "tests", "c", "keyset_index33_main.cpp"), "-o", exe])
    p = subprocess.run([exe, "0x5ec9", "1", "0xfeedfacecafebeef", "0x0123456789abcdef"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok 4 seeds"), p.stdout + p.stderr[-2000:]
