"""SHA-2 digests on the device and the ECDSA verification calls that take messages (csrc/digest.hip, csrc/sha2.h).

The digest kernel is compared with hashlib for all three algorithms and both input forms, at the lengths where the padding
turns (55/56 and 119/120 for the 64-byte blocks, 111/112 for SHA-512's 128-byte blocks), in a ragged batch whose lanes
differ in block count, at every alignment of an item's start, and on both sides of the capacity below which a workgroup
stages its stretch of the blob in LDS.  The verification calls must give, bit for bit, what their digest siblings give on
the host-computed digests - on every ladder the dispatch can pick - and what the fixtures and the CPU oracle expect."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import pyref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
N = R.N
b32 = R.b32
H = bytes.fromhex

LEN32 = [0, 1, 31, 32, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 183, 184]      # SHA-256, SHA-256d
LEN64 = [0, 1, 110, 111, 112, 113, 127, 128, 129, 239, 240, 241, 256]                      # SHA-512
ERR_ARG = -3


def sha256d(m):
    return hashlib.sha256(hashlib.sha256(m).digest()).digest()


def href(S, alg, m, out_len=32):
    if alg == S.HASH_SHA256:
        return hashlib.sha256(m).digest()
    if alg == S.HASH_SHA256D:
        return sha256d(m)
    return hashlib.sha512(m).digest()[:out_len]


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


def knobs(eng, small, mid, ks=0, comb=0):
    eng.set_small_batch_max(small)
    eng.set_mid_batch_max(mid)
    eng.set_keyset_small_batch_max(ks)
    eng.set_keyset_comb_small_batch_max(comb)


LADDERS = {"wave": (4096, 0), "quad": (0, 32768), "lane": (0, 0)}


def _rows(vals):
    return np.frombuffer(b"".join(vals), np.uint8).reshape(len(vals), -1).copy()


def check_digests(S, eng, msgs, alg, out_len=32):
    got = eng.digest_batch(msgs, alg, out_len)
    assert got.shape == (len(msgs), out_len)
    for i, m in enumerate(msgs):
        assert bytes(got[i]) == href(S, alg, m, out_len), (alg, i, len(m))


# ---- the digest kernel against hashlib ---------------------------------------------------------------------------

@pytest.mark.parametrize("alg", [0, 1, 2])
def test_digest_lengths_both_forms(S, eng, alg):
    rng = random.Random(2300 + alg)
    lens = LEN64 if alg == S.HASH_SHA512 else LEN32
    out_len = 64 if alg == S.HASH_SHA512 else 32
    check_digests(S, eng, [rng.randbytes(n) for n in lens], alg, out_len)              # one blob with offsets
    if alg == S.HASH_SHA512:
        check_digests(S, eng, [rng.randbytes(n) for n in lens], alg, 32)               # its leftmost 32 bytes
    for n in lens:                                                                     # n strings of msg_len bytes
        a = np.frombuffer(rng.randbytes(3 * n), np.uint8).reshape(3, n).copy()
        got = eng.digest_batch(a, alg, out_len)
        assert [bytes(g) for g in got] == [href(S, alg, bytes(r), out_len) for r in a], n


@pytest.mark.parametrize("alg", [0, 1, 2])
def test_digest_ragged_batch(S, eng, alg):
    """700 items (the last workgroup is not full), lengths drawn from the lists, so lanes of one wave differ in block
    count; offsets that do not start at 0; zero-length items between long ones; item starts at every residue mod 16."""
    rng = random.Random(2310 + alg)
    lens = LEN64 if alg == S.HASH_SHA512 else LEN32
    out_len = 64 if alg == S.HASH_SHA512 else 32
    msgs = [rng.randbytes(rng.choice(lens)) for _ in range(700)]
    for i in range(40, 700, 97):                                  # empty items between long ones
        msgs[i - 1], msgs[i], msgs[i + 1] = rng.randbytes(lens[-1]), b"", rng.randbytes(lens[-1])
    lead = rng.randbytes(37)                                      # bytes in front of the first item: msg_offsets[0] != 0
    offs = np.zeros(701, np.uint64)
    offs[0] = len(lead)
    offs[1:] = len(lead) + np.cumsum([len(m) for m in msgs])
    assert {int(o) % 16 for o in offs[:-1]} == set(range(16))
    blob = np.frombuffer(lead + b"".join(msgs), np.uint8)
    got = eng.digest_batch((blob, offs), alg, out_len)
    for i, m in enumerate(msgs):
        assert bytes(got[i]) == href(S, alg, m, out_len), (i, len(m))


def test_digest_staging_boundary(S, eng):
    """A workgroup's stretch of lo..hi bytes is staged in LDS when (hi - (lo & ~15)) + 16 <= cap, else read in place: totals
    on both sides of that turn, cap - 1, cap and cap + 1 themselves, and one item of 2 cap bytes."""
    cap = S.digest_caps()
    assert cap >= 4096 and cap % 16 == 0
    rng = random.Random(2320)
    for total in (cap - 17, cap - 16, cap - 15, cap - 1, cap, cap + 1):
        each = total // 256
        lens = [each] * 255 + [total - 255 * each]
        for alg in (S.HASH_SHA256, S.HASH_SHA512):
            check_digests(S, eng, [rng.randbytes(n) for n in lens], alg)
    big = [rng.randbytes(5), rng.randbytes(2 * cap), b"", rng.randbytes(70)]
    for alg in (S.HASH_SHA256, S.HASH_SHA256D, S.HASH_SHA512):
        check_digests(S, eng, big, alg)
    # 300 items: the first workgroup holds the long item and reads in place, the second one stages
    check_digests(S, eng, big + [rng.randbytes(33) for _ in range(296)], S.HASH_SHA256)


@pytest.mark.parametrize("alg,out_len,stride", [(0, 32, 48), (0, 32, 40), (1, 32, 33), (2, 32, 64), (2, 64, 80), (2, 64, 67)])
def test_digest_output_stride(S, eng, alg, out_len, stride):
    rng = random.Random(2330 + stride)
    msgs = [rng.randbytes(rng.randrange(0, 200)) for _ in range(300)]
    out = np.full((300, stride), 0xA5, np.uint8)
    eng.digest_batch(msgs, alg, out_len, out_stride=stride, out=out)
    for i, m in enumerate(msgs):
        assert bytes(out[i, :out_len]) == href(S, alg, m, out_len), i
    assert (out[:, out_len:] == 0xA5).all()


# ---- verification from messages ----------------------------------------------------------------------------------

def wycheproof(oracle, name):
    """(pub, msgs, digests, r, s, expected) of the cases whose signature parses (the others are never valid)"""
    msgs = load_golden("wycheproof_ecdsa_msgs.json")[name]
    pub, m, dig, rr, ss, exp = [], [], [], [], [], []
    for c in load_golden(f"wycheproof_ecdsa_{name}.json")["cases"]:
        rs = oracle.parse_asn1_signature(H(c["sig"]))
        if rs is None:
            assert not c["valid"]
            continue
        pub.append(H(c["pub"])[1:]), m.append(H(msgs[str(c["tcId"])])), dig.append(H(c["digest"])[:32])
        rr.append(rs[0]), ss.append(rs[1]), exp.append(int(c["valid"]))
    return pub, m, dig, rr, ss, exp


@pytest.mark.parametrize("ladder", sorted(LADDERS))
@pytest.mark.parametrize("name", ["sha256", "sha512"])
def test_wycheproof_from_messages(S, eng, oracle, name, ladder):
    pub, m, dig, rr, ss, exp = wycheproof(oracle, name)
    assert sum(exp) == {"sha256": 164, "sha512": 233}[name]
    knobs(eng, *LADDERS[ladder])
    alg = S.HASH_SHA256 if name == "sha256" else S.HASH_SHA512
    got = eng.ecdsa_verify_messages_batch(pub, m, rr, ss, alg)
    assert got.tolist() == exp
    assert got.tolist() == eng.ecdsa_verify_batch(pub, dig, rr, ss).tolist()


def test_rfc6979_messages(S, eng, oracle):
    knobs(eng, 4096, 32768)
    pub, m, rr, ss = [], [], [], []
    for c in load_golden("rfc6979.json")["cases"]:
        pub.append(oracle.scalar_base_mult_vartime(H(c["private"]))[1:])
        m.append(c["message"].encode())
        r, s = oracle.parse_asn1_signature(H(c["sig"]))
        rr.append(r), ss.append(s)
    assert eng.ecdsa_verify_messages_batch(pub, m, rr, ss, S.HASH_SHA256).all()
    assert not eng.ecdsa_verify_messages_batch(pub, m, rr, ss, S.HASH_SHA256D).any()
    assert not eng.ecdsa_verify_messages_batch(pub, m, rr, ss, S.HASH_SHA512).any()


def signed_batch(S, oracle, seed, n, nkeys, digest_of, outside_every=0, damage_every=8):
    """n variable-length messages signed over digest_of(message) under nkeys keys (every outside_every-th one under a key of
    its own), one in damage_every damaged: the message, s, or r.  -> dict of arrays, the keys, and the oracle's verdicts on
    the host-computed digests."""
    rng = random.Random(seed)
    d = [rng.randrange(1, N) for _ in range(nkeys)]
    keys = [oracle.scalar_base_mult_vartime(b32(x))[1:] for x in d]
    pub, kidx, msgs, dig, rr, ss = [], [], [], [], [], []
    for i in range(n):
        k = rng.randrange(nkeys)
        x, q = d[k], keys[k]
        if outside_every and i % outside_every == 1:
            x = rng.randrange(1, N)
            q, k = oracle.scalar_base_mult_vartime(b32(x))[1:], 0xFFFFFFFF
        m = rng.randbytes(rng.choice([0, 1, 20, 32, 55, 56, 64, 100, 119, 120, 200]))
        sig = None
        while sig is None:
            sig = S.ct_ecdsa_sign_raw(b32(x), digest_of(m), rng.randbytes(32))
        r, s = sig[0], sig[1]
        if damage_every and i % damage_every == damage_every // 2:
            kind = (i // damage_every) % 3
            if kind == 0: m = m + b"!"
            elif kind == 1: s = b32((int.from_bytes(s, "big") + 1) % N or 1)
            else: r = b32(int.from_bytes(r, "big") ^ 2 or 1)
        pub.append(q), kidx.append(k), msgs.append(m), dig.append(digest_of(m)), rr.append(r), ss.append(s)
    w = {"pub": _rows(pub), "kidx": np.array(kidx, np.uint32), "msgs": msgs, "dig": _rows(dig), "r": _rows(rr), "s": _rows(ss), "keys": _rows(keys)}
    w["exp"] = oracle.ecdsa_verify_batch(w["pub"], w["dig"], w["r"], w["s"])
    assert 0 < int(w["exp"].sum()) < n
    return w


@pytest.mark.parametrize("ladder", sorted(LADDERS))
def test_sha256d_messages(S, eng, oracle, ladder):
    w = signed_batch(S, oracle, 2340, 300, 5, sha256d)
    knobs(eng, *LADDERS[ladder])
    got = eng.ecdsa_verify_messages_batch(w["pub"], w["msgs"], w["r"], w["s"], S.HASH_SHA256D)
    assert got.tolist() == w["exp"].tolist()
    assert int(got.sum()) == 300 - len(range(4, 300, 8))
    # the same signatures are over another digest under plain SHA-256
    assert not eng.ecdsa_verify_messages_batch(w["pub"], w["msgs"], w["r"], w["s"], S.HASH_SHA256).any()


@pytest.fixture(scope="module")
def keyset_batch(S, oracle):
    return signed_batch(S, oracle, 2350, 300, 8, lambda m: hashlib.sha256(m).digest(), outside_every=4)


@pytest.mark.parametrize("rows", [True, False])
@pytest.mark.parametrize("layout", ["JOINT5", "COMB"])
def test_keysets_from_messages(S, eng, oracle, keyset_batch, layout, rows):
    """A set of 8 keys with an index: by key index and by key bytes (a quarter of the items under keys outside the set),
    with the row-ladder knobs on and at 0; the verdicts are the digest siblings', bit for bit, and the oracle's."""
    w = keyset_batch
    ks = eng.keyset_create(w["keys"], getattr(S, "KEYSET_" + layout))
    try:
        ks.index_create()
        if rows:
            knobs(eng, 3072, 32768, ks=4096, comb=4096)      # (by key bytes, a call this small is the plain call: its ladders)
        else:
            knobs(eng, 0, 0, ks=0, comb=0)
        inside = w["kidx"] != 0xFFFFFFFF
        exp_idx = np.where(inside, w["exp"], 0).astype(np.uint8)      # an index outside the set verifies false
        got = eng.ecdsa_verify_messages_batch_keyset(ks, w["kidx"], w["msgs"], w["r"], w["s"], S.HASH_SHA256)
        sib = eng.ecdsa_verify_batch_keyset(ks, w["kidx"], w["dig"], w["r"], w["s"])
        if rows:
            assert eng.last_keyset_ladder() == (S.KEYSET_LADDER_ROW_COMB if layout == "COMB" else S.KEYSET_LADDER_ROW)
        assert got.tolist() == sib.tolist() == exp_idx.tolist()
        got = eng.ecdsa_verify_messages_batch_bykey(ks, w["pub"], w["msgs"], w["r"], w["s"], S.HASH_SHA256)
        sib = eng.ecdsa_verify_batch_bykey(ks, w["pub"], w["dig"], w["r"], w["s"])
        assert got.tolist() == sib.tolist() == w["exp"].tolist()
    finally:
        ks.close()


def test_four_tickets_in_flight(S, eng, oracle):
    knobs(eng, 3072, 32768)
    batches = [signed_batch(S, oracle, 2360 + t, 257, 3, lambda m: hashlib.sha256(m).digest(), damage_every=3 + t) for t in range(4)]
    tickets = [eng.ecdsa_verify_messages_batch_submit(w["pub"], w["msgs"], w["r"], w["s"], S.HASH_SHA256) for w in batches]
    for t, w in reversed(list(zip(tickets, batches))):
        assert t.wait().tolist() == w["exp"].tolist()


# ---- refusals: S2K_ERR_ARG before anything is launched, outputs untouched, the next good call right --------------

def test_refusals(S, eng, oracle, keyset_batch):
    import torch
    w = keyset_batch
    n = 300
    lib, h = S.load_library(), eng._h
    knobs(eng, 3072, 32768, ks=2048, comb=0)
    ks = eng.keyset_create(w["keys"], S.KEYSET_JOINT5)
    ks.index_create()
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(m) for m in w["msgs"]])
    blob = np.frombuffer(b"".join(w["msgs"]), np.uint8)
    bad_offs = offs.copy()
    bad_offs[150], bad_offs[151] = offs[151], offs[150]                 # decreases once
    assert bad_offs[150] > bad_offs[151]
    valid = np.full(n, 0x5A, np.uint8)
    out = np.full((n, 64), 0x5A, np.uint8)
    p = lambda a: a.ctypes.data                                         # noqa: E731
    pub, kidx, r, s = w["pub"], w["kidx"], w["r"], w["s"]
    big = 1 << 31

    def host_forms(alg, msgs, mo, mlen, rr=p(r)):
        """every host form that verifies, with these message arguments: all must refuse"""
        t = C.c_uint64(7)
        rcs = [lib.s2k_ecdsa_verify_messages_batch(h, n, p(pub), alg, msgs, mo, mlen, rr, p(s), 0, p(valid)),
               lib.s2k_ecdsa_verify_messages_batch_submit(h, n, p(pub), alg, msgs, mo, mlen, rr, p(s), 0, p(valid), C.byref(t)),
               lib.s2k_ecdsa_verify_messages_batch_keyset(h, ks._k, n, p(kidx), alg, msgs, mo, mlen, rr, p(s), 0, p(valid)),
               lib.s2k_ecdsa_verify_messages_batch_keyset_bykey(h, ks._k, n, p(pub), alg, msgs, mo, mlen, rr, p(s), 0, p(valid))]
        assert t.value == 0
        return rcs

    try:
        for args in ((7, p(blob), p(offs), 0), (-1, p(blob), p(offs), 0),        # unknown alg
                     (0, p(blob), p(bad_offs), 0),                               # offsets decrease
                     (0, None, p(offs), 0), (0, None, None, 5),                  # no message buffer
                     (0, p(blob), None, big), (2, p(blob), None, big + 5)):      # msg_len >= 2^31
            assert host_forms(*args) == [ERR_ARG] * 4, args
            assert lib.s2k_digest_batch(h, args[0], n, args[1], args[2], args[3], p(out), 32) == ERR_ARG, args
        assert host_forms(0, p(blob), p(offs), 0, rr=None) == [ERR_ARG] * 4      # a NULL signature array
        assert lib.s2k_ecdsa_verify_messages_batch(h, n, p(pub), 0, p(blob), p(offs), 0, p(r), p(s), 0, None) == ERR_ARG
        assert lib.s2k_digest_batch(h, 0, n, p(blob), p(offs), 0, None, 32) == ERR_ARG
        for alg, out_len in ((0, 64), (1, 64), (0, 31), (2, 48), (2, 0)):        # out_len: 32, or 64 with SHA-512
            assert lib.s2k_digest_batch(h, alg, n, p(blob), p(offs), 0, p(out), out_len) == ERR_ARG, (alg, out_len)
        # the device forms, on real device buffers: the same argument checks (their offsets are the caller's precondition)
        d = {k: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
             for k, a in (("pub", pub), ("kidx", kidx), ("blob", blob), ("offs", offs), ("r", r), ("s", s), ("valid", valid), ("out", out))}
        torch.cuda.synchronize()
        q = {k: v.data_ptr() for k, v in d.items()}
        for alg, msgs, mo, mlen in ((7, q["blob"], q["offs"], 0), (0, None, q["offs"], 0), (0, None, None, 5), (0, q["blob"], None, big)):
            assert lib.s2k_ecdsa_verify_messages_batch_device(h, n, q["pub"], alg, msgs, mo, mlen, q["r"], q["s"], 0, q["valid"], None) == ERR_ARG
            assert lib.s2k_ecdsa_verify_messages_batch_keyset_device(h, ks._k, n, q["kidx"], alg, msgs, mo, mlen, q["r"], q["s"], 0, q["valid"], None) == ERR_ARG
            assert lib.s2k_ecdsa_verify_messages_batch_keyset_bykey_device(h, ks._k, n, q["pub"], alg, msgs, mo, mlen, q["r"], q["s"], 0, q["valid"], None) == ERR_ARG
            assert lib.s2k_digest_batch_device(h, alg, n, msgs, mo, mlen, q["out"], 32, None) == ERR_ARG
        assert lib.s2k_ecdsa_verify_messages_batch_device(h, n, q["pub"], 0, q["blob"], q["offs"], 0, None, q["s"], 0, q["valid"], None) == ERR_ARG
        assert lib.s2k_digest_batch_device(h, 0, n, q["blob"], q["offs"], 0, q["out"], 64, None) == ERR_ARG
        torch.cuda.synchronize()
        assert (d["valid"].cpu().numpy() == 0x5A).all() and (d["out"].cpu().numpy() == 0x5A).all()
        assert (valid == 0x5A).all() and (out == 0x5A).all()
        # n == 0 succeeds and writes nothing, whatever else is passed
        assert lib.s2k_ecdsa_verify_messages_batch(h, 0, None, 0, None, None, 0, None, None, 0, None) == 0
        assert lib.s2k_digest_batch(h, 2, 0, None, None, 0, None, 64) == 0
        # ... and the context is as good as before
        inside = kidx != 0xFFFFFFFF
        assert eng.ecdsa_verify_messages_batch(pub, w["msgs"], r, s).tolist() == w["exp"].tolist()
        assert eng.ecdsa_verify_messages_batch_keyset(ks, kidx, (blob, offs), r, s).tolist() == np.where(inside, w["exp"], 0).tolist()
        assert eng.ecdsa_verify_messages_batch_bykey(ks, pub, w["msgs"], r, s).tolist() == w["exp"].tolist()
        assert [bytes(g) for g in eng.digest_batch(w["msgs"])] == [bytes(x) for x in w["dig"]]
    finally:
        ks.close()
