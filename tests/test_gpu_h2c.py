"""Hashing to the curve on the device (csrc/h2c.hip) through the C-ABI: the RFC 9380 vectors the reference ships
(tests/golden/h2c.json) and the big-integer model tests/h2c_model.py, which follows the RFC in affine coordinates with its
inversions - not the device's fraction form.  All batches are small (n <= 2048); the model's answers are computed once per
module and shared."""
import ctypes as C
import random

import numpy as np
import pytest

import h2c_model as M
import pyref
from conftest import load_golden

pytestmark = pytest.mark.gpu
S2K_ERR_ARG = -3
P = M.P


@pytest.fixture(scope="module")
def S():
    import secp256k1_voi_amd as S
    return S


@pytest.fixture(scope="module")
def eng(S):
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return load_golden("h2c.json")


def _rec(pt):
    return np.frombuffer(pyref.enc65(pt), dtype=np.uint8)


def _model(suite_ro, msg, dst):
    return (M.hash_to_curve if suite_ro else M.encode_to_curve)(msg, dst)[0]


# ---- 1. RFC vectors through the C-ABI ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["ro", "nu"])
def test_rfc_suite_vectors(eng, golden, key):
    g = golden[key]
    dst = bytes.fromhex(g["dst"])
    msgs = [bytes.fromhex(v["msg"]) for v in g["vectors"]]
    assert len(msgs) == 5 and max(len(m) for m in msgs) >= 512      # ("a512_" and 512 letters: several blocks)
    got = eng.hash_to_curve(msgs, dst) if key == "ro" else eng.encode_to_curve(msgs, dst)
    assert got.shape == (5, 65)
    for v, rec in zip(g["vectors"], got):
        assert rec.tobytes().hex() == "04" + v["P"][0] + v["P"][1]
    # the mapped points themselves (Q0, Q1 / Q) from the u the vectors state
    for v in g["vectors"]:
        u = b"".join(int(x, 16).to_bytes(32, "big") for x in v["u"])
        q = eng.map_to_curve(u, 32, 1)
        want = [v["Q0"], v["Q1"]] if key == "ro" else [v["Q"]]
        assert [r.tobytes().hex() for r in q] == ["04" + w[0] + w[1] for w in want]


@pytest.mark.parametrize("key", ["expand_short_dst", "expand_long_dst"])
def test_rfc_expand_vectors(eng, golden, key):
    g = golden[key]
    dst = bytes.fromhex(g["dst"])
    lens = sorted({t["len_in_bytes"] for t in g["tests"]})
    assert lens == [32, 128] and len(g["tests"]) == 10
    for ln in lens:
        ts = [t for t in g["tests"] if t["len_in_bytes"] == ln]
        got = eng.expand_message_xmd([bytes.fromhex(t["msg"]) for t in ts], dst, ln)
        assert [r.tobytes().hex() for r in got] == [t["uniform_bytes"] for t in ts]


# ---- 2. padding and batch-boundary sweep --------------------------------------------------------------------------------
DST_LENS = [1, 16, 49, 255, 256, 300]


def _sweep_dst(n):
    return bytes((11 * i + n) & 0xff for i in range(n))


def _sweep_msg(dl, ln):
    return bytes((i * 37 + ln * 5 + dl) & 0xff for i in range(ln))


@pytest.fixture(scope="module")
def sweep_msgs():
    """786 messages: lengths 0..130, six different fillings of each"""
    msgs = [_sweep_msg(dl, ln) for dl in DST_LENS for ln in range(131)]
    assert len(msgs) == 786
    return msgs


@pytest.mark.parametrize("suite_ro", [True, False])
@pytest.mark.parametrize("dst_len", DST_LENS)
def test_padding_sweep_offsets_form(S, eng, sweep_msgs, suite_ro, dst_len):
    """every residue of the SHA padding, for b_0 and for the b_i: 786 items in one call of the offsets form (message
    lengths 0..130, six times), for each tag length - short, oversize (hashed), and the longest that is not"""
    dst = _sweep_dst(dst_len)
    blob, offs = S._concat(sweep_msgs)
    got = (eng.hash_to_curve if suite_ro else eng.encode_to_curve)((blob, offs), dst)
    assert got.shape == (786, 65)
    want = np.stack([_rec(_model(suite_ro, m, dst)) for m in sweep_msgs])
    assert np.array_equal(got, want)


@pytest.fixture(scope="module")
def fixed_model():
    """fixed-length form: 257 messages of 32 bytes and the empty message, both suites, tag of 49 bytes"""
    dst = _sweep_dst(49)
    rng = random.Random(20)
    msgs = [rng.randbytes(32) for _ in range(257)]
    out = {}
    for ro in (True, False):
        out[(ro, 32)] = np.stack([_rec(_model(ro, m, dst)) for m in msgs])
        out[(ro, 0)] = _rec(_model(ro, b"", dst))
    return dst, msgs, out


@pytest.mark.parametrize("suite_ro", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_fixed_length_form(S, eng, fixed_model, suite_ro, n):
    dst, msgs, want = fixed_model
    lib = eng._lib
    suite = S.H2C_SSWU_RO if suite_ro else S.H2C_SSWU_NU
    blob = np.frombuffer(b"".join(msgs[:n]), dtype=np.uint8)
    out = np.zeros((n, 65), dtype=np.uint8)
    assert lib.s2k_hash_to_curve_batch(eng._h, suite, n, dst, len(dst), blob.ctypes.data, None, 32, out.ctypes.data) == 0
    assert np.array_equal(out, want[(suite_ro, 32)][:n])
    out0 = np.full((n, 65), 0xee, dtype=np.uint8)
    assert lib.s2k_hash_to_curve_batch(eng._h, suite, n, dst, len(dst), None, None, 0, out0.ctypes.data) == 0
    assert np.array_equal(out0, np.tile(want[(suite_ro, 0)], (n, 1)))


def test_empty_batch(S, eng):
    lib = eng._lib
    assert lib.s2k_hash_to_curve_batch(eng._h, S.H2C_SSWU_RO, 0, b"tag", 3, None, None, 0, None) == 0
    assert eng.hash_to_curve([], b"tag").shape == (0, 65)


# ---- 3. map_to_curve edges ------------------------------------------------------------------------------------------------
def _enc(value, length):
    return int(value).to_bytes(length, "big")


def _edge_values(length):
    """integers that fit `length` bytes and reduce to the interesting field elements"""
    root = pyref.sqrt_p(pow(11, -1, P))
    vals = [0, root, P - root, 1, P - 1]                       # u = 0, Z u^2 = -1 (both roots), u = 1, u = -1
    vals += [P, P + 1, 2**256 - 1]                             # 32-byte inputs >= p: reduced, not refused
    if length > 32:
        top = 2 ** (8 * length)
        k = (top - 1 - root) // P                                # the largest multiples of p that still fit
        vals += [top - 1, P << (8 * (length - 32)), k * P, k * P + root]
    return vals


@pytest.fixture(scope="module")
def map_cases():
    cases = {}
    for length in (32, 48, 64):
        rng = random.Random(1000 + length)
        singles = [_enc(v, length) for v in _edge_values(length)]
        if length == 64:
            singles.append(b"\xff" * 64)
        singles += [rng.randbytes(length) for _ in range(200)]
        want1 = np.stack([_rec(M.set_uniform_bytes(b)) for b in singles])
        u0 = [rng.randrange(1, P) for _ in range(4)]
        pairs = [(_enc(u, length), _enc(u, length)) for u in u0]                      # u1 = u0: the sum is a doubling
        pairs += [(_enc(u, length), _enc(P - u, length)) for u in u0]                 # u1 = -u0: the identity
        pairs += [(_enc(0, length), _enc(0, length)), (_enc(0, length), _enc(P, length))]
        pairs += [(singles[i], singles[i + 1]) for i in range(0, len(singles) - 1, 2)]
        want2 = np.stack([_rec(M.map_to_curve_sum(a + b, length, 2)) for a, b in pairs])
        cases[length] = (singles, want1, pairs, want2)
    return cases


@pytest.mark.parametrize("length", [32, 48, 64])
def test_map_to_curve_edges(eng, map_cases, length):
    singles, want1, pairs, want2 = map_cases[length]
    got1 = eng.map_to_curve(singles, length, 1)
    assert np.array_equal(got1, want1)
    got2 = eng.map_to_curve([a + b for a, b in pairs], length, 2)
    assert np.array_equal(got2, want2)
    for k in range(4, 8):                                       # Q + (-Q): 65 zero bytes
        assert got2[k].tobytes() == bytes(65)
    for rec in list(got1) + list(got2):
        if rec[0] != 0:
            assert rec[0] == 4 and pyref.on_curve(pyref.dec65(rec.tobytes()))
    assert all(r[0] == 4 for r in got1)                        # a single mapped point is never the identity


# ---- 4. device form -------------------------------------------------------------------------------------------------------
def test_device_form_feeds_multi_scalar_mult(S, eng):
    torch = pytest.importorskip("torch")
    rng = random.Random(64)
    dst = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_RO_"
    msgs = [rng.randbytes(rng.randrange(0, 90)) for _ in range(64)]
    scalars = [rng.randrange(pyref.N) for _ in range(64)]
    blob, offs = S._concat(msgs)
    dev = torch.device("cuda:0")
    d_blob = torch.from_numpy(blob.copy()).to(dev)
    d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
    d_rec = torch.zeros(64 * 65, dtype=torch.uint8, device=dev)
    d_k = torch.from_numpy(np.frombuffer(b"".join(pyref.b32(k) for k in scalars), dtype=np.uint8).copy()).to(dev)
    d_sum = torch.zeros(65, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    eng.hash_to_curve_device(S.H2C_SSWU_RO, 64, dst, d_blob.data_ptr(), d_offs.data_ptr(), 0, int(offs[-1]), d_rec.data_ptr(), stream)
    eng.multi_scalar_mult_device(64, d_k.data_ptr(), d_rec.data_ptr(), d_sum.data_ptr(), stream)
    torch.cuda.synchronize()
    want_pts = [M.hash_to_curve(m, dst)[0] for m in msgs]
    acc = None
    for k, q in zip(scalars, want_pts):
        acc = pyref.add(acc, pyref.mul(k, q))
    assert d_sum.cpu().numpy().tobytes() == pyref.enc65(acc)
    host = eng.hash_to_curve(msgs, dst)
    assert np.array_equal(d_rec.cpu().numpy().reshape(64, 65), host)
    assert np.array_equal(host, np.stack([_rec(q) for q in want_pts]))


@pytest.mark.parametrize("offsets,stated,bad", [
    ([0, 16, 32, 48, 64], 40, {2, 3}),          # the stated size is smaller than the last offsets
    ([0, 16, 8, 48, 64], 64, {1}),              # one decreasing pair
    ([8, 16, 32, 48, 64], 64, {0}),             # offsets that do not start at 0
])
def test_device_form_bad_offsets(S, eng, offsets, stated, bad):
    """Device offsets cannot be checked before the launch: a lane whose range decreases or leaves [0, total_msg_bytes)
    reads no message byte, writes the identity record and raises the status word, which is S2K_ERR_ARG at the call's one
    synchronisation; the other lanes hash what their ranges name.  The buffer really holds 64 bytes, so every offset
    here lies inside it whatever the kernel did with it."""
    torch = pytest.importorskip("torch")
    dst = b"QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_NU_"
    blob = bytes(range(64))
    dev = torch.device("cuda:0")
    d_blob = torch.tensor(list(blob), dtype=torch.uint8, device=dev)
    d_offs = torch.tensor(offsets, dtype=torch.int64, device=dev)
    d_rec = torch.full((4 * 65,), 0xa5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    rc = eng._lib.s2k_hash_to_curve_batch_device(eng._h, S.H2C_SSWU_NU, 4, dst, len(dst), d_blob.data_ptr(), d_offs.data_ptr(), 0,
                                                 stated, d_rec.data_ptr(), stream)
    assert rc == S2K_ERR_ARG
    got = d_rec.cpu().numpy().reshape(4, 65)
    for i in range(4):
        want = bytes(65) if i in bad else pyref.enc65(M.encode_to_curve(blob[offsets[i]:offsets[i + 1]], dst)[0])
        assert got[i].tobytes() == want, i
    # the context still works afterwards
    assert eng.encode_to_curve([b"abc"], dst)[0].tobytes() == pyref.enc65(M.encode_to_curve(b"abc", dst)[0])


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(S, eng):
    lib, h = eng._lib, eng._h
    out = np.full(8161 * 2, 0xa5, dtype=np.uint8)
    msg = np.arange(64, dtype=np.uint8)
    o, m = out.ctypes.data, msg.ctypes.data
    good = np.array([0, 32, 64], dtype=np.uint64)
    down = np.array([0, 40, 32], dtype=np.uint64)
    late = np.array([8, 32, 64], dtype=np.uint64)
    RO = S.H2C_SSWU_RO
    calls = [
        lambda: lib.s2k_hash_to_curve_batch(h, RO, 2, b"x", 0, m, good.ctypes.data, 0, o),          # dst_len == 0
        lambda: lib.s2k_expand_message_xmd_batch(h, 2, b"x", 0, m, good.ctypes.data, 0, 32, o),
        lambda: lib.s2k_map_to_curve_batch(h, 1, 1, 31, m, o),                                      # len 31, 65
        lambda: lib.s2k_map_to_curve_batch(h, 1, 1, 65, m, o),
        lambda: lib.s2k_map_to_curve_batch(h, 1, 0, 32, m, o),                                      # count 0, 3
        lambda: lib.s2k_map_to_curve_batch(h, 1, 3, 32, m, o),
        lambda: lib.s2k_expand_message_xmd_batch(h, 2, b"tag", 3, m, good.ctypes.data, 0, 0, o),    # len_in_bytes 0, 8161
        lambda: lib.s2k_expand_message_xmd_batch(h, 2, b"tag", 3, m, good.ctypes.data, 0, 8161, o),
        lambda: lib.s2k_hash_to_curve_batch(h, RO, 2, b"tag", 3, m, down.ctypes.data, 0, o),        # decreasing host offsets
        lambda: lib.s2k_expand_message_xmd_batch(h, 2, b"tag", 3, m, down.ctypes.data, 0, 32, o),
        lambda: lib.s2k_hash_to_curve_batch(h, RO, 2, b"tag", 3, m, late.ctypes.data, 0, o),        # offsets that do not start at 0
        lambda: lib.s2k_hash_to_curve_batch(h, 7, 2, b"tag", 3, m, good.ctypes.data, 0, o),         # unknown suite
        lambda: lib.s2k_hash_to_curve_batch(h, RO, 2, b"tag", 3, m, good.ctypes.data, 0, None),     # null buffers with n > 0
        lambda: lib.s2k_hash_to_curve_batch(h, RO, 2, b"tag", 3, None, good.ctypes.data, 0, o),
        lambda: lib.s2k_hash_to_curve_batch(h, RO, 2**31, b"tag", 3, m, None, 0, o),                # n > 2^31 - 1
        lambda: lib.s2k_hash_to_curve_batch_device(h, RO, 2, b"x", 0, None, None, 0, 0, o, None),   # device form: before any launch
        lambda: lib.s2k_hash_to_curve_batch_device(h, RO, 4, b"tag", 3, m, None, 32, 64, o, None),  # n * msg_len > total
    ]
    for i, call in enumerate(calls):
        assert call() == S2K_ERR_ARG, i
        assert bool(np.all(out == 0xa5)), i
    # the context still works afterwards
    assert eng.encode_to_curve([b"abc"], b"tag")[0].tobytes() == pyref.enc65(M.encode_to_curve(b"abc", b"tag")[0])


def test_longest_expansion(eng):
    """len_in_bytes = 8160 (ell = 255, the most the RFC allows) for one message"""
    msg, dst = b"the longest expansion", b"QUUX-V01-CS02-with-expander-SHA256-128"
    got = eng.expand_message_xmd([msg], dst, 8160)
    assert got.shape == (1, 8160) and got[0].tobytes() == M.expand_message_xmd(msg, dst, 8160)
    # ... and lengths that end inside a block of the output
    for ln in (1, 31, 33, 95, 96):
        got = eng.expand_message_xmd([msg, b""], dst, ln)
        assert got[0].tobytes() == M.expand_message_xmd(msg, dst, ln) and got[1].tobytes() == M.expand_message_xmd(b"", dst, ln)
