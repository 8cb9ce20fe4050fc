"""Sanitizer run of the host half of hashing to the curve (csrc/h2c_host.h: SHA-256 and DST_prime take caller-supplied
lengths): a stand-alone program, built for the host with AddressSanitizer + UndefinedBehaviorSanitizer and run on the CPU.
No device code is involved and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest


def test_h2c_host_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "h2c_san")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(root, "secp256k1_voi_amd", "csrc"),
                           os.path.join(root, "tests", "c", "h2c_sanitize_main.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok"), p.stdout + p.stderr[-2000:]
