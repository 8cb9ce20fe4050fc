"""Keccak-256 addresses on the device (csrc/address.hip): of 65-byte key records, and of the keys recovered from signatures,
from digests or straight from messages.

k_keccak_address is compared with tests/keccak_model.py; the recovery forms with ecdsa_recover_batch on the same inputs - ok
bit for bit, the addresses the model's of that call's keys - on every path the recovery dispatch has; the messages form with
the digest form on the model's digests; the device forms with the host forms, with rows and records at odd addresses and
guard bytes around the rows."""
import hashlib
import random

import numpy as np
import pytest

import ecdsa_rlc_model as E
import keccak_model as K
import pyref as R

pytestmark = pytest.mark.gpu
N, P = R.N, R.P
b32 = R.b32
NREC = 330                                  # no multiple of 256, 64 or 4
LENS = [0, 1, 7, 8, 9, 31, 32, 64, 134, 135, 136, 137, 143, 144, 271, 272, 273, 408]
ADDR_OF_ONE = bytes.fromhex("7e5f4552091a69125d5dfcb7b8c2659029395bdf")
PATHS = {"wave": (4096, 0, False), "quad": (0, 32768, False), "lane": (0, 0, False), "complete": (0, 0, True)}
KINDS = ["r flipped", "s shifted", "digest flipped", "r = 0", "s = 0", "r >= n", "v >= 4", "r no abscissa"]
ERR_ARG = -3


@pytest.fixture(scope="module")
def S():
    import secp256k1_voi_amd as S
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


def model_addresses(pub65, ok=None):
    """what s2k_keccak_address_batch promises, from the model"""
    out = np.zeros((len(pub65), 20), np.uint8)
    for i, rec in enumerate(pub65):
        if rec[0] == 4 and (ok is None or ok[i]):
            out[i] = np.frombuffer(K.address(bytes(rec[1:])), np.uint8)
    return out


@pytest.fixture(scope="module")
def batch(oracle):
    """330 recoverable signatures over ragged messages, signed twice: over the model's Keccak-256 of the message and over
    hashlib's SHA-256.  Item 1 is the high-x tuple (bit 1 of v set); every fourth item is damaged, each kind at least once;
    secret 1 signs every seventh item."""
    rng = random.Random(2450)

    def bm(k):
        q = oracle.scalar_base_mult_vartime(b32(k))
        return int.from_bytes(q[1:33], "big"), int.from_bytes(q[33:], "big")

    secrets = [1] + [rng.randrange(1, N) for _ in range(6)]
    no_abscissa = next(x for x in range(5, 1000) if R.lift_x(x, 0) is None)
    hx = E.high_x_tuple(2451)
    msgs = [rng.randbytes(LENS[(5 * i + 3) % len(LENS)]) for i in range(NREC)]
    msgs[8] = b""
    out = {"msgs": None}
    for name, digest_of in (("keccak", K.keccak256), ("sha256", lambda m: hashlib.sha256(m).digest())):
        rr, ss, vv, mm, kinds = [], [], [], [], []
        r2 = random.Random(2452)
        for i in range(NREC):
            m = msgs[i]
            r, s, v = E.sign_recoverable(secrets[i % 7], digest_of(m), r2.randrange(1, N), base_mult=bm)
            kind = None
            if i == 1:
                (_, r, s), v = hx, 2
            elif i % 4 == 2:
                kind = KINDS[(i // 4) % 8]
                if kind == "r flipped": r = (r ^ (1 << r2.randrange(250))) % N or 1
                elif kind == "s shifted": s = (s + 1 + r2.randrange(1000)) % N or 1
                elif kind == "digest flipped": m = m + b"?"
                elif kind == "r = 0": r = 0
                elif kind == "s = 0": s = 0
                elif kind == "r >= n": r = N + r % 1000
                elif kind == "v >= 4": v = 4 + (i & 3)
                else: r = no_abscissa
            rr.append(b32(r)), ss.append(b32(s)), vv.append(v), mm.append(m), kinds.append(kind)
        assert set(KINDS) <= set(kinds)
        if out["msgs"] is None:
            out["msgs"], out["kinds"] = mm, kinds
        assert out["msgs"] == mm
        out[name] = {"dig": _rows([digest_of(m) for m in mm]), "r": _rows(rr), "s": _rows(ss), "v": np.array(vv, np.uint8)}
    assert b"" in out["msgs"] and out["keccak"]["v"][1] == 2
    return out


def knobs(eng, small, mid):
    eng.set_small_batch_max(small)
    eng.set_mid_batch_max(mid)


# ---- records to addresses -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def records(oracle):
    rng = random.Random(2460)
    recs = []
    for i in range(NREC):
        if i == 5:
            recs.append(bytes(oracle.scalar_base_mult_vartime(b32(1))))          # the key of secret 1
        elif i % 11 == 3:
            recs.append(bytes(65))                                               # the zero record (no key)
        elif i % 13 == 6:
            recs.append(bytes([rng.choice([0, 2, 3, 5, 0xff])]) + rng.randbytes(64))   # another first byte
        elif i % 3 == 0:
            recs.append(bytes(oracle.scalar_base_mult_vartime(b32(rng.randrange(1, N)))))
        else:
            recs.append(b"\x04" + rng.randbytes(64))                             # hashed as given: no curve check
    return _rows(recs)


def test_keccak_address_batch_against_model(eng, records):
    exp = model_addresses(records)
    assert bytes(exp[5]) == ADDR_OF_ONE and not exp[3].any() and not exp[6].any() and exp[0].any()
    got = eng.keccak_address_batch(records)
    assert got.shape == (NREC, 20) and np.array_equal(got, exp)
    ok = np.ones(NREC, np.uint8)
    ok[[0, 7, 64, 255, 256, 329]] = 0
    ok[100:110] = 0
    ok[200] = 0x80                                                               # any non-zero byte counts
    got = eng.keccak_address_batch(records, ok)
    assert np.array_equal(got, model_addresses(records, ok)) and not got[0].any() and got[200].any()
    knobs(eng, 0, 0)                                                             # the same through the DMA route of the host form
    assert np.array_equal(eng.keccak_address_batch(records, ok), model_addresses(records, ok))
    knobs(eng, 3072, 32768)


# ---- recovery to addresses ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", sorted(PATHS))
def test_recover_address_every_path(eng, batch, path):
    b = batch["keccak"]
    small, mid, complete = PATHS[path]
    knobs(eng, small, mid)
    try:
        pub, ok = eng.ecdsa_recover_batch(b["dig"], b["r"], b["s"], b["v"], force_complete=complete)
        addr, ok2 = eng.ecdsa_recover_address_batch(b["dig"], b["r"], b["s"], b["v"], force_complete=complete)
    finally:
        knobs(eng, 3072, 32768)
    assert ok2.tobytes() == ok.tobytes()
    assert np.array_equal(addr, model_addresses(pub, ok))
    assert not addr[ok == 0].any() and 0 < int((ok != 0).sum()) < NREC
    for i, kind in enumerate(batch["kinds"]):
        if kind in ("r = 0", "s = 0", "r >= n", "v >= 4", "r no abscissa"):
            assert ok[i] == 0, (i, kind)
        elif kind is None:
            assert ok[i] == 1, i
            if i % 7 == 0 and i != 1:
                assert bytes(addr[i]) == ADDR_OF_ONE, i                          # signed by secret 1
    assert ok[1] == 1                                                            # the high-x item has a key
    assert sum(1 for i, k in enumerate(batch["kinds"]) if k is None and i % 7 == 0) > 10


@pytest.mark.parametrize("path", ["wave", "lane"])
def test_recover_address_from_messages(S, eng, batch, path):
    small, mid, _ = PATHS[path]
    knobs(eng, small, mid)
    try:
        for name, alg in (("keccak", S.HASH_KECCAK256), ("sha256", S.HASH_SHA256)):
            b = batch[name]
            addr, ok = eng.ecdsa_recover_address_batch(b["dig"], b["r"], b["s"], b["v"])
            got, gok = eng.ecdsa_recover_address_messages_batch(batch["msgs"], b["r"], b["s"], b["v"], alg)
            assert gok.tobytes() == ok.tobytes() and got.tobytes() == addr.tobytes(), name
            assert bytes(addr[7]) == ADDR_OF_ONE
        # the signatures over SHA-256 digests, hashed as Keccak-256: keys, but other keys
        b = batch["sha256"]
        other, _ = eng.ecdsa_recover_address_messages_batch(batch["msgs"], b["r"], b["s"], b["v"])
        assert bytes(other[7]) != ADDR_OF_ONE and other[7].any()
    finally:
        knobs(eng, 3072, 32768)


def test_device_forms_at_odd_addresses(S, eng, batch, records):
    """torch buffers on a stream of the caller's; the rows start one byte past a 16-byte boundary between guard bytes (the
    only place a wide store past a 20-byte row would show), the records at an odd address."""
    import torch
    b = batch["keccak"]
    n = NREC
    want_addr, want_ok = eng.ecdsa_recover_address_batch(b["dig"], b["r"], b["s"], b["v"])
    st = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()      # noqa: E731
    d = {k: dev(b[k]) for k in ("dig", "r", "s", "v")}
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(m) for m in batch["msgs"]])
    d_blob, d_offs = dev(np.frombuffer(b"".join(batch["msgs"]), np.uint8)), dev(offs)

    def guarded():
        t = torch.full((65 + 20 * n + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        return t

    def rows_of(t):
        h = t.cpu().numpy()
        assert (h[:65] == 0xAA).all() and (h[65 + 20 * n:] == 0xAA).all()
        return h[65:65 + 20 * n].reshape(n, 20)

    out1, out2, out3 = guarded(), guarded(), guarded()
    ok1, ok2 = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(1 + 65 * n, dtype=torch.uint8, device="cuda")
    d_rec[1:] = dev(records)
    assert (d_rec.data_ptr() + 1) % 2 == 1
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        s = st.cuda_stream
        eng.ecdsa_recover_address_batch_device(n, d["dig"].data_ptr(), d["r"].data_ptr(), d["s"].data_ptr(), d["v"].data_ptr(),
                                               out1.data_ptr() + 65, ok1.data_ptr(), stream=s)
        eng.ecdsa_recover_address_messages_batch_device(n, S.HASH_KECCAK256, d_blob.data_ptr(), d_offs.data_ptr(), 0, d["r"].data_ptr(),
                                                        d["s"].data_ptr(), d["v"].data_ptr(), out2.data_ptr() + 65, ok2.data_ptr(), stream=s)
        eng.keccak_address_batch_device(n, d_rec.data_ptr() + 1, None, out3.data_ptr() + 65, stream=s)
    st.synchronize()
    assert np.array_equal(rows_of(out1), want_addr) and ok1.cpu().numpy().tobytes() == want_ok.tobytes()
    assert np.array_equal(rows_of(out2), want_addr) and ok2.cpu().numpy().tobytes() == want_ok.tobytes()
    assert np.array_equal(rows_of(out3), model_addresses(records))


def test_refusals(S, eng, batch, records):
    lib, h = S.load_library(), eng._h
    b = batch["keccak"]
    n = NREC
    p = lambda a: a.ctypes.data                                         # noqa: E731
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(m) for m in batch["msgs"]])
    blob = np.frombuffer(b"".join(batch["msgs"]), np.uint8)
    bad_offs = offs.copy()
    bad_offs[150], bad_offs[151] = offs[151], offs[150]
    assert bad_offs[150] > bad_offs[151]
    addr, ok = np.full((n, 20), 0x5A, np.uint8), np.full(n, 0x5A, np.uint8)
    dig, r, s, v = b["dig"], b["r"], b["s"], b["v"]
    big = 1 << 31
    # a NULL buffer
    assert lib.s2k_keccak_address_batch(h, n, None, None, p(addr)) == ERR_ARG
    assert lib.s2k_keccak_address_batch(h, n, p(records), None, None) == ERR_ARG
    assert lib.s2k_keccak_address_batch(None, n, p(records), None, p(addr)) == ERR_ARG
    for hole in range(6):
        args = [p(dig), p(r), p(s), p(v), 0, p(addr), p(ok)]
        args[hole if hole < 4 else hole + 1] = None
        assert lib.s2k_ecdsa_recover_address_batch(h, n, *args) == ERR_ARG, hole
    for hole in range(5):
        args = [p(r), p(s), p(v), 0, p(addr), p(ok)]
        args[hole if hole < 3 else hole + 1] = None
        assert lib.s2k_ecdsa_recover_address_messages_batch(h, n, 3, p(blob), p(offs), 0, *args) == ERR_ARG, hole
    # the message arguments: an unknown alg, msg_len = 2^31, no blob, offsets that decrease
    for alg, msgs, mo, mlen in ((7, p(blob), p(offs), 0), (3, p(blob), None, big), (3, None, p(offs), 0), (3, p(blob), p(bad_offs), 0)):
        assert lib.s2k_ecdsa_recover_address_messages_batch(h, n, alg, msgs, mo, mlen, p(r), p(s), p(v), 0, p(addr), p(ok)) == ERR_ARG, (alg, mlen)
    # the device forms check their arguments the same way (no pointer is followed)
    assert lib.s2k_ecdsa_recover_address_messages_batch_device(h, n, 7, p(blob), p(offs), 0, p(r), p(s), p(v), 0, p(addr), p(ok), None) == ERR_ARG
    assert lib.s2k_ecdsa_recover_address_messages_batch_device(h, n, 3, p(blob), None, big, p(r), p(s), p(v), 0, p(addr), p(ok), None) == ERR_ARG
    assert lib.s2k_ecdsa_recover_address_batch_device(h, n, p(dig), p(r), p(s), p(v), 0, None, p(ok), None) == ERR_ARG
    assert lib.s2k_keccak_address_batch_device(h, n, None, None, p(addr), None) == ERR_ARG
    assert lib.s2k_keccak_address_batch_device(h, 1 << 30, p(records), None, p(addr), None) == ERR_ARG
    assert (addr == 0x5A).all() and (ok == 0x5A).all()
    # n == 0 succeeds and writes nothing, whatever else is passed
    assert lib.s2k_keccak_address_batch(h, 0, None, None, None) == 0
    assert lib.s2k_ecdsa_recover_address_batch(h, 0, None, None, None, None, 0, None, None) == 0
    assert lib.s2k_ecdsa_recover_address_messages_batch(h, 0, 3, None, None, 0, None, None, None, 0, None, None) == 0
    assert lib.s2k_ecdsa_recover_address_messages_batch_device(h, 0, 3, None, None, 0, None, None, None, 0, None, None, None) == 0
    # ... and the context is as good as before
    got, gok = eng.ecdsa_recover_address_messages_batch(batch["msgs"], r, s, v)
    want, wok = eng.ecdsa_recover_address_batch(dig, r, s, v)
    assert got.tobytes() == want.tobytes() and gok.tobytes() == wok.tobytes() and bytes(want[7]) == ADDR_OF_ONE
