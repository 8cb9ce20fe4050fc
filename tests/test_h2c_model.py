"""Hashing to the curve, CPU side: the big-integer model of RFC 9380 (tests/h2c_model.py) against the reference's own
vectors (tests/golden/h2c.json), and the host half of the library - s2k_h2c_dst_prime and the argument checks that need
no device - against the model."""
import ctypes as C
import hashlib
import os
import struct
import subprocess
import sys

import pytest

import h2c_model as M
import pyref
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S2K_ERR_ARG = -3


@pytest.fixture(scope="module")
def golden():
    return load_golden("h2c.json")


def _hex_pt(pt):
    return ["%064x" % c for c in pt]


@pytest.mark.parametrize("key", ["ro", "nu"])
def test_model_reproduces_suite_vectors(golden, key):
    g = golden[key]
    dst = bytes.fromhex(g["dst"])
    assert len(g["vectors"]) == 5
    for v in g["vectors"]:
        msg = bytes.fromhex(v["msg"])
        if key == "ro":
            pt, u, (q0, q1) = M.hash_to_curve(msg, dst)
            assert _hex_pt(q0) == v["Q0"] and _hex_pt(q1) == v["Q1"]
        else:
            pt, u, (q,) = M.encode_to_curve(msg, dst)
            assert _hex_pt(q) == v["Q"]
        assert ["%064x" % x for x in u] == v["u"]
        assert _hex_pt(pt) == v["P"] and pyref.on_curve(pt)


@pytest.mark.parametrize("key", ["expand_short_dst", "expand_long_dst"])
def test_model_reproduces_expand_vectors(golden, key):
    g = golden[key]
    dst = bytes.fromhex(g["dst"])
    assert len(g["tests"]) == 10
    for t in g["tests"]:
        assert M.expand_message_xmd(bytes.fromhex(t["msg"]), dst, t["len_in_bytes"]).hex() == t["uniform_bytes"]
        assert M.dst_prime(dst).hex() == t["DST_prime"]


def test_model_edges():
    """the exceptional branch of SSWU (u = 0 and Z u^2 = -1), Q + Q and Q - Q, inputs that need the reduction"""
    root = pyref.sqrt_p(pow(11, -1, M.P))
    assert root is not None and (M.Z * root * root + 1) % M.P == 0
    for u in (0, root, M.P - root, 1, M.P - 1):
        q = M.map_to_curve(u)
        assert q is not None and pyref.on_curve(q)
    u0 = 12345
    b0, b1 = u0.to_bytes(32, "big"), (M.P - u0).to_bytes(32, "big")
    assert M.map_to_curve_sum(b0 + b1, 32, 2) is None                       # sgn0 flips with u: Q1 = -Q0
    assert M.map_to_curve_sum(b0 + b0, 32, 2) == pyref.add(M.map_to_curve(u0), M.map_to_curve(u0))
    assert M.set_uniform_bytes(M.P.to_bytes(32, "big")) == M.map_to_curve(0)
    assert M.set_uniform_bytes(b"\xff" * 64) == M.map_to_curve((2**512 - 1) % M.P)


def test_fixture_generator_is_reproducible(tmp_path):
    """tests/golden/make_h2c_fixtures.py gives the committed h2c.json byte for byte (where the reference tree is at hand)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_fixtures
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(make_fixtures.REF, "secec", "h2c", "testdata")):
        pytest.skip("reference tree not present")
    import shutil
    gen = tmp_path / "golden"
    gen.mkdir()
    for fn in ("make_fixtures.py", "make_h2c_fixtures.py"):
        shutil.copy(os.path.join(ROOT, "tests", "golden", fn), gen / fn)
    subprocess.check_call([sys.executable, str(gen / "make_h2c_fixtures.py")], stdout=subprocess.DEVNULL)
    assert (gen / "h2c.json").read_bytes() == open(os.path.join(ROOT, "tests", "golden", "h2c.json"), "rb").read()


def test_zpad_midstate_constant():
    """csrc/h2c.hip starts b_0 from the SHA-256 state after the 64 zero bytes of Z_pad: re-derive the constant it states"""
    src = open(os.path.join(ROOT, "secp256k1_voi_amd", "csrc", "h2c.hip")).read()
    at = src.index("H2C_ZPAD_MIDSTATE[8] = {")
    words = [int(x.strip().rstrip("u"), 16) for x in src[src.index("{", at) + 1:src.index("}", at)].split(",")]
    K = [int(x, 16) for x in (
        "428a2f98 71374491 b5c0fbcf e9b5dba5 3956c25b 59f111f1 923f82a4 ab1c5ed5 d807aa98 12835b01 243185be 550c7dc3 72be5d74 "
        "80deb1fe 9bdc06a7 c19bf174 e49b69c1 efbe4786 0fc19dc6 240ca1cc 2de92c6f 4a7484aa 5cb0a9dc 76f988da 983e5152 a831c66d "
        "b00327c8 bf597fc7 c6e00bf3 d5a79147 06ca6351 14292967 27b70a85 2e1b2138 4d2c6dfc 53380d13 650a7354 766a0abb 81c2c92e "
        "92722c85 a2bfe8a1 a81a664b c24b8b70 c76c51a3 d192e819 d6990624 f40e3585 106aa070 19a4c116 1e376c08 2748774c 34b0bcb5 "
        "391c0cb3 4ed8aa4a 5b9cca4f 682e6ff3 748f82ee 78a5636f 84c87814 8cc70208 90befffa a4506ceb bef9a3f7 c67178f2").split()]
    iv = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
    m32 = 0xffffffff

    def rotr(x, n):
        return ((x >> n) | (x << (32 - n))) & m32

    def compress(st, block):
        w = list(struct.unpack(">16I", block))
        for i in range(16, 64):
            s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
            s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
            w.append((w[i - 16] + s0 + w[i - 7] + s1) & m32)
        a, b, c, d, e, f, g, h = st
        for i in range(64):
            t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i]) & m32
            t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & m32
            h, g, f, e, d, c, b, a = g, f, e, (d + t1) & m32, c, b, a, (t1 + t2) & m32
        return [(x + y) & m32 for x, y in zip(st, [a, b, c, d, e, f, g, h])]

    mid = compress(iv, bytes(64))
    assert words == mid
    # ... and the compression itself against hashlib: Z_pad || "abc" is one more block
    tail = b"abc\x80" + bytes(52) + struct.pack(">Q", 67 * 8)
    assert b"".join(struct.pack(">I", x) for x in compress(mid, tail)) == hashlib.sha256(bytes(64) + b"abc").digest()


# ---- the built library, host side only -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def S():
    import secp256k1_voi_amd as S
    if not os.path.exists(S.LIB_PATH):
        S.build()
    return S


@pytest.mark.parametrize("dst_len", [1, 49, 255, 256, 300])
def test_dst_prime_matches_model(S, golden, dst_len):
    dst = bytes((7 * i + dst_len) & 0xff for i in range(dst_len))
    got = S.h2c_dst_prime(dst)
    assert got == M.dst_prime(dst)
    assert len(got) == (dst_len + 1 if dst_len <= 255 else 33)


def test_dst_prime_matches_fixtures(S, golden):
    for key in ("expand_short_dst", "expand_long_dst"):
        dst = bytes.fromhex(golden[key]["dst"])
        assert S.h2c_dst_prime(dst).hex() == golden[key]["tests"][0]["DST_prime"]
    for key in ("ro", "nu"):
        dst = bytes.fromhex(golden[key]["dst"])
        assert len(dst) == 49 and S.h2c_dst_prime(dst) == dst + b"\x31"


def test_dst_prime_refuses_empty_tag(S):
    with pytest.raises(ValueError):
        S.h2c_dst_prime(b"")
    lib = S.load_library()
    out, n = C.create_string_buffer(b"\xaa" * 256, 256), C.c_size_t(77)
    assert lib.s2k_h2c_dst_prime(b"x", 0, out, C.byref(n)) == S2K_ERR_ARG
    assert lib.s2k_h2c_dst_prime(None, 5, out, C.byref(n)) == S2K_ERR_ARG
    assert out.raw == b"\xaa" * 256 and n.value == 77


def test_null_context_is_refused_without_a_device(S):
    """every new entry point that takes a context refuses a null one with S2K_ERR_ARG before it touches a device (this
    machine may have none), and leaves the output alone"""
    lib = S.load_library()
    out = C.create_string_buffer(b"\x55" * 256, 256)
    msg, dst = C.create_string_buffer(b"m" * 64, 64), b"tag"
    o = C.addressof(out)
    m = C.addressof(msg)
    assert lib.s2k_expand_message_xmd_batch(None, 1, dst, 3, m, None, 32, 32, o) == S2K_ERR_ARG
    assert lib.s2k_map_to_curve_batch(None, 1, 1, 48, m, o) == S2K_ERR_ARG
    assert lib.s2k_hash_to_curve_batch(None, S.H2C_SSWU_RO, 1, dst, 3, m, None, 32, o) == S2K_ERR_ARG
    assert lib.s2k_hash_to_curve_batch(None, S.H2C_SSWU_NU, 0, dst, 3, None, None, 0, None) == S2K_ERR_ARG
    assert lib.s2k_hash_to_curve_batch_device(None, S.H2C_SSWU_RO, 1, dst, 3, m, None, 32, 32, o, None) == S2K_ERR_ARG
    assert out.raw == b"\x55" * 256
    assert b"ctx is NULL" in lib.s2k_last_error(None)


def test_python_layer_checks_lengths_before_the_call(S):
    """Engine's h2c methods check their arguments in Python (no context needed to see that: the checks come first)"""
    class Stub(S.Engine):
        def __init__(self):          # no context: any C call would fail loudly
            self._lib, self._h = None, None

        def __del__(self):
            pass

    e = Stub()
    with pytest.raises(ValueError):
        e.hash_to_curve([b"m"], b"")
    with pytest.raises(ValueError):
        e.encode_to_curve([b"m"], b"")
    for bad in (0, 8161):
        with pytest.raises(ValueError):
            e.expand_message_xmd([b"m"], b"tag", bad)
    for length, count in ((31, 1), (65, 1), (48, 0), (48, 3)):
        with pytest.raises(ValueError):
            e.map_to_curve(bytes(length * max(count, 1)), length, count)
    with pytest.raises(ValueError):
        e.map_to_curve(bytes(47), 48)                          # not a multiple of count * length
    import numpy as np
    blob = np.zeros(8, dtype=np.uint8)
    for offs in ([1, 4], [0, 5, 3], [0, 9]):
        with pytest.raises(ValueError):
            e.hash_to_curve((blob, np.array(offs, dtype=np.uint64)), b"tag")
