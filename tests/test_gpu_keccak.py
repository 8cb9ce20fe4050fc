"""Keccak-256 and SHA3-256 on the device (csrc/keccak.h, k_digest_keccak in csrc/digest.hip) as hash ids 3 and 4 of the digest
call and of the ECDSA verification calls that take messages.

The reference is tests/keccak_model.py for Keccak-256, and hashlib.sha3_256 and the model for SHA3-256.  Lengths are the
ones where a 136-byte sponge turns: both padding bytes in one byte (135), a whole extra block (136, 272, 408), lane
boundaries (7, 8, 9, 143, 144); in a ragged batch whose lanes differ in block count, at every alignment of an item's start,
and on both sides of the capacity below which a workgroup stages its stretch of the blob in LDS.  The verification calls
must give, bit for bit, what their digest siblings give on the model's digests."""
import functools
import hashlib
import random

import numpy as np
import pytest

import keccak_model as K
import pyref as R

pytestmark = pytest.mark.gpu
N = R.N
b32 = R.b32
LENS = [0, 1, 7, 8, 9, 31, 32, 64, 134, 135, 136, 137, 143, 144, 271, 272, 273, 408]
ALGS = [3, 4]
ERR_ARG = -3


@functools.lru_cache(maxsize=None)
def href(alg, m):
    if alg == 4:
        d = hashlib.sha3_256(m).digest()
        assert d == K.sha3_256(m)
        return d
    return K.keccak256(m)


@pytest.fixture(scope="module")
def S():
    import secp256k1_voi_amd as S
    assert (S.HASH_KECCAK256, S.HASH_SHA3_256) == (3, 4)
    return S


@pytest.fixture(scope="module")
def eng(S):
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    e = S.Engine(0)
    yield e
    e.close()


def _rows(vals):
    return np.frombuffer(b"".join(vals), np.uint8).reshape(len(vals), -1).copy()


def check_digests(eng, msgs, alg):
    got = eng.digest_batch(msgs, alg, 32)
    assert got.shape == (len(msgs), 32)
    for i, m in enumerate(msgs):
        assert bytes(got[i]) == href(alg, m), (alg, i, len(m))


@pytest.mark.parametrize("alg", ALGS)
def test_keccak_lengths_both_forms(eng, alg):
    rng = random.Random(2400 + alg)
    check_digests(eng, [rng.randbytes(n) for n in LENS], alg)                           # one blob with offsets
    for n in LENS:                                                                      # n strings of msg_len bytes
        a = np.frombuffer(rng.randbytes(3 * n), np.uint8).reshape(3, n).copy()
        got = eng.digest_batch(a, alg, 32)
        assert [bytes(g) for g in got] == [href(alg, bytes(r)) for r in a], n
    # the published vectors, so that the model is not the only witness
    want = {3: "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45", 4: hashlib.sha3_256(b"abc").hexdigest()}[alg]
    assert bytes(eng.digest_batch([b"abc"], alg)[0]).hex() == want


@pytest.mark.parametrize("alg", ALGS)
def test_keccak_ragged_batch(eng, alg):
    """700 items (the last workgroup is not full), lengths drawn from the list, so lanes of one wave differ in block count;
    offsets that do not start at 0; zero-length items between long ones; item starts at every residue mod 16."""
    rng = random.Random(2410 + alg)
    msgs = [rng.randbytes(rng.choice(LENS)) for _ in range(700)]
    for i in range(40, 700, 97):                                  # empty items between long ones
        msgs[i - 1], msgs[i], msgs[i + 1] = rng.randbytes(LENS[-1]), b"", rng.randbytes(LENS[-1])
    lead = rng.randbytes(37)                                      # bytes in front of the first item: msg_offsets[0] != 0
    offs = np.zeros(701, np.uint64)
    offs[0] = len(lead)
    offs[1:] = len(lead) + np.cumsum([len(m) for m in msgs])
    assert {int(o) % 16 for o in offs[:-1]} == set(range(16))
    blob = np.frombuffer(lead + b"".join(msgs), np.uint8)
    got = eng.digest_batch((blob, offs), alg, 32)
    for i, m in enumerate(msgs):
        assert bytes(got[i]) == href(alg, m), (i, len(m))


def test_keccak_staging_boundary(S, eng):
    """A workgroup's stretch is staged in LDS when (hi - (lo & ~15)) + 16 <= cap, else read in place: totals on both sides of
    that turn, and one item of 2 cap bytes among short ones."""
    cap = S.digest_caps()
    assert cap >= 4096 and cap % 16 == 0
    rng = random.Random(2420)
    for total in (cap - 17, cap - 16, cap - 15, cap - 1, cap, cap + 1):
        each = total // 256
        lens = [each] * 255 + [total - 255 * each]
        for alg in ALGS:
            check_digests(eng, [rng.randbytes(n) for n in lens], alg)
    big = [rng.randbytes(5), rng.randbytes(2 * cap), b"", rng.randbytes(70)]
    for alg in ALGS:
        check_digests(eng, big, alg)
    check_digests(eng, big + [rng.randbytes(33) for _ in range(296)], 3)     # the second workgroup stages, the first does not


@pytest.mark.parametrize("alg,stride", [(3, 48), (4, 40), (3, 33)])
def test_keccak_output_stride(eng, alg, stride):
    rng = random.Random(2430 + stride)
    msgs = [rng.randbytes(rng.randrange(0, 200)) for _ in range(300)]
    out = np.full((300, stride), 0xA5, np.uint8)
    eng.digest_batch(msgs, alg, 32, out_stride=stride, out=out)
    for i, m in enumerate(msgs):
        assert bytes(out[i, :32]) == href(alg, m), i
    assert (out[:, 32:] == 0xA5).all()


def test_keccak_refusals(S, eng):
    lib, h = S.load_library(), eng._h
    msgs = np.frombuffer(bytes(range(64)), np.uint8).copy()
    out = np.full((2, 64), 0x5A, np.uint8)
    for alg, out_len in ((3, 64), (4, 64), (5, 32)):
        assert lib.s2k_digest_batch(h, alg, 2, msgs.ctypes.data, None, 32, out.ctypes.data, out_len) == ERR_ARG, (alg, out_len)
        assert lib.s2k_debug_digest_strided(h, alg, 2, msgs.ctypes.data, None, 32, out.ctypes.data, out_len, 64) == ERR_ARG, (alg, out_len)
    assert (out == 0x5A).all()
    check_digests(eng, [bytes(msgs[:32]), bytes(msgs[32:])], 3)              # ... and the context is as good as before


# ---- the verification calls that take messages --------------------------------------------------------------------

@pytest.fixture(scope="module")
def signed(S, oracle):
    """96 signatures over 8 keys on the model's Keccak-256 of ragged messages, every eighth damaged (message, s, r)"""
    rng = random.Random(2440)
    d = [rng.randrange(1, N) for _ in range(8)]
    keys = [oracle.scalar_base_mult_vartime(b32(x))[1:] for x in d]
    pub, kidx, msgs, dig, rr, ss = [], [], [], [], [], []
    for i in range(96):
        k = i % 8
        m = rng.randbytes(LENS[i % len(LENS)])
        sig = None
        while sig is None:
            sig = S.ct_ecdsa_sign_raw(b32(d[k]), K.keccak256(m), rng.randbytes(32))
        r, s = sig[0], sig[1]
        if i % 8 == 4:
            kind = (i // 8) % 3
            if kind == 0: m = m + b"!"
            elif kind == 1: s = b32((int.from_bytes(s, "big") + 1) % N or 1)
            else: r = b32(int.from_bytes(r, "big") ^ 2 or 1)
        pub.append(keys[k]), kidx.append(k), msgs.append(m), dig.append(K.keccak256(m)), rr.append(r), ss.append(s)
    w = {"pub": _rows(pub), "kidx": np.array(kidx, np.uint32), "msgs": msgs, "dig": _rows(dig), "r": _rows(rr), "s": _rows(ss), "keys": _rows(keys)}
    w["exp"] = oracle.ecdsa_verify_batch(w["pub"], w["dig"], w["r"], w["s"])
    assert int(w["exp"].sum()) == 96 - 12
    return w


def test_keccak_messages_calls(S, eng, signed):
    w = signed
    A = S.HASH_KECCAK256
    sib = eng.ecdsa_verify_batch(w["pub"], w["dig"], w["r"], w["s"])
    assert sib.tolist() == w["exp"].tolist()
    assert eng.ecdsa_verify_messages_batch(w["pub"], w["msgs"], w["r"], w["s"], A).tolist() == sib.tolist()
    assert eng.ecdsa_verify_messages_batch_submit(w["pub"], w["msgs"], w["r"], w["s"], A).wait().tolist() == sib.tolist()
    assert not eng.ecdsa_verify_messages_batch(w["pub"], w["msgs"], w["r"], w["s"], S.HASH_SHA256).any()
    ks = eng.keyset_create(w["keys"], S.KEYSET_JOINT5)
    try:
        ks.index_create()
        got = eng.ecdsa_verify_messages_batch_keyset(ks, w["kidx"], w["msgs"], w["r"], w["s"], A)
        assert got.tolist() == eng.ecdsa_verify_batch_keyset(ks, w["kidx"], w["dig"], w["r"], w["s"]).tolist() == sib.tolist()
        got = eng.ecdsa_verify_messages_batch_bykey(ks, w["pub"], w["msgs"], w["r"], w["s"], A)
        assert got.tolist() == eng.ecdsa_verify_batch_bykey(ks, w["pub"], w["dig"], w["r"], w["s"]).tolist() == sib.tolist()
    finally:
        ks.close()
