"""Encoded ECDSA batches over a key set: the compressed-key probe of the index (s2k_keyset_lookup with key_bytes 33:
k_ksi_lookup<33>), the key-set parse step (k_parse_encoded_keyset, k_decompress_list) and the calls that join them with the
set's ladders (s2k_ecdsa_verify_encoded_batch_keyset[_submit], s2k_ctx_last_encoded_keyset_stats).

The 33-byte lookup is exact against a Python dict over the set's VALID keys (both parities, random strings, the off-curve
key whose parity names a point the set does not hold, X >= p, bad prefixes); the encoded call gives the plain encoded call's
and the oracle's verdicts byte for byte in every layout, encoding and flag, with the hits of either key length and the square
roots counted; exceptional lanes end on the worklist; a call in pieces hands its short last piece to the plain path; small
calls are the plain call; tickets equal their synchronous counterparts."""
import os
import random

import numpy as np
import pytest

import pyref as R
import test_gpu_comb as TC
from test_gpu_keyset_bykey import lookup_case  # noqa: F401  (the 1000-key fixture: real keys, negations, duplicates, off-curve, X >= p)

pytestmark = pytest.mark.gpu
N, P = R.N, R.P
b32 = R.b32
NONE = 0xFFFFFFFF
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768
NSIG = 4096 + 37
LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _int(b):
    return int.from_bytes(bytes(b), "big")


def _on_curve(key):
    x, y = _int(key[:32]), _int(key[32:])
    return x < P and y < P and (y * y - x * x * x - 7) % P == 0


def _compressed(key):
    """02 / 03 || X of a 64-byte key, by the parity of its Y (for a key off the curve: the bytes that name another point)"""
    return bytes([2 + (int(key[63]) & 1)]) + bytes(key[:32])


def _der(rb, sb):
    body = b""
    for x in (_int(rb), _int(sb)):
        bb = x.to_bytes((x.bit_length() + 8) // 8 or 1, "big")
        body += b"\x02" + bytes([len(bb)]) + bb
    return b"\x30" + bytes([len(body)]) + body


# ---- 1. the 33-byte lookup is exact ----
@pytest.fixture(scope="module")
def lookup33_case(lookup_case):
    keys = lookup_case[0]
    valid = np.array([_on_curve(k) for k in keys])
    truth = {}
    for i, k in enumerate(keys):
        if valid[i]:
            truth.setdefault((int(k[63]) & 1, bytes(k[:32])), i)
    rng = np.random.default_rng(2001)
    off = [i for i, k in enumerate(keys) if not valid[i] and _int(k[:32]) < P]           # the off-curve key and its duplicate
    big = [i for i, k in enumerate(keys) if _int(k[:32]) >= P]
    assert len(off) >= 1 and len(big) >= 1 and valid.sum() == 1000 - len(off) - len(big)
    good = np.nonzero(valid)[0]
    paired = [i for i in good if (1 - (int(keys[i][63]) & 1), bytes(keys[i][:32])) in truth]      # Q with -Q in the set too
    assert len(paired) >= 20
    nq = 5000
    kind = rng.permutation(nq) % 10          # 0-3 a key of the set; 4 its X with the other parity; 5-6 random; 7 trap; 8 X >= p; 9 bad prefix
    kind[0] = 0                              # (the call of one key: a hit)
    q = np.zeros((nq, 33), np.uint8)
    for j in range(nq):
        kd = kind[j]
        if kd <= 4 or kd == 9:
            k = keys[paired[j % len(paired)]] if (kd == 4 and j % 2 == 0) else keys[good[rng.integers(0, len(good))]]
            c = bytearray(_compressed(k))
            if kd == 4:
                c[0] ^= 1
            if kd == 9:
                c[0] = (0x00, 0x04, 0x05, 0x01)[j % 4]
        elif kd <= 6:
            c = bytearray(rng.integers(0, 256, size=33, dtype=np.uint8).tobytes())
            c[0] = 2 + (j & 1)
        elif kd == 7:
            # the trap: 02 / 03 || X by the parity of the off-curve Y names the VALID point (X, that parity), which is not the
            # set's entry; the other prefix names its negation
            c = bytearray(_compressed(keys[off[j % len(off)]]))
            if j % 3 == 0:
                c[0] ^= 1
        else:
            c = bytearray(_compressed(keys[big[j % len(big)]]))
            c[0] = 2 + (j & 1)
        q[j] = np.frombuffer(bytes(c), np.uint8)
    exp = np.array([truth.get((int(c[0]) & 1, bytes(c[1:])), NONE) if c[0] in (2, 3) else NONE for c in q], np.uint32)
    for kd in range(10):
        assert (kind == kd).sum() >= 10
    assert (exp[kind <= 3] != NONE).all() and (exp[kind >= 5] == NONE).all()
    assert (exp[kind == 4] != NONE).sum() >= 10 and (exp[kind == 4] == NONE).sum() >= 10    # -Q is in the set for ten keys only
    # every trap expectation is a miss unless the set also held the valid point: it does not
    off_x = {bytes(keys[i][:32]) for i in off}
    assert not any(x in off_x for (_, x) in truth) and (exp[kind == 7] == NONE).all()
    return keys, valid, q, exp


def test_lookup33_is_exact(eng, lookup33_case):
    import torch
    import secp256k1_voi_amd as S
    keys, valid, q, exp = lookup33_case
    ks = eng.keyset_create(keys, S.KEYSET_COMB)
    try:
        ks.index_create(10)
        assert np.array_equal(ks.valid_keys() != 0, valid)
        for n in (1, 257, 5000):
            qq = np.ascontiguousarray(q[:n])
            assert np.array_equal(eng.keyset_lookup(ks, qq, key_bytes=33), exp[:n]), n
            assert np.array_equal(eng.keyset_lookup(ks, qq, key_bytes=33, stride=33), exp[:n]), n
            rec36 = np.concatenate([np.full((n, 3), 0xEE, np.uint8), qq], axis=1)        # records of 36 bytes, the key at offset 3
            assert np.array_equal(eng.keyset_lookup(ks, rec36, key_bytes=33, stride=36, offset=3), exp[:n]), n
        dev = torch.device("cuda", 0)
        n = 5000
        d_q = torch.from_numpy(q).to(dev)
        d_out = torch.zeros(n, dtype=torch.int32, device=dev)
        eng.keyset_lookup_device(ks, n, d_q.data_ptr(), d_out.data_ptr(), key_bytes=33, stride=33)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().view(np.uint32), exp)
        assert eng.keyset_lookup(ks, np.zeros((0, 33), np.uint8), key_bytes=33).shape == (0,)
        with pytest.raises(S.EngineError):
            eng.keyset_lookup_device(ks, n, d_q.data_ptr(), d_out.data_ptr(), key_bytes=48)
        with pytest.raises(S.EngineError):
            eng.keyset_lookup_device(ks, n, d_q.data_ptr(), d_out.data_ptr(), key_bytes=33, stride=32)
        with pytest.raises(ValueError):
            eng.keyset_lookup(ks, q, key_bytes=48)
    finally:
        ks.close()


# ---- 2. verdicts ----
TRAP = 5                                     # the key of the set that is replaced by an off-curve key of the same X


@pytest.fixture(scope="module")
def enc_case(eng, oracle):
    """4096 + 37 signatures of 80 keys (the first 64 in the set), built as test_gpu_keyset_bykey.fused_case: a tenth damaged in
    the low 16 bytes of r, s or the digest (the encodings stay well formed), every other valid signature with the high s;
    keys 3 and 7 (in the set) and 70 (outside) are no public keys.  Keys alternate between the compressed and the uncompressed
    encoding (a key that is no point has only the uncompressed one).  The signatures of key TRAP are turned into signatures
    under -Q = (X, p - Y) - (n - e, r, n - s) verifies under -Q iff (e, r, s) does under Q - and presented compressed, while
    the set lists (X, Y ^ 1) in its place: off the curve, with the parity of p - Y.  40 malformed items follow.
    Reference verdicts per (encoding, reject_malleable, bip0066): the plain encoded call (thresholds off) and the oracle on
    the decoded arrays (0 for malformed items)."""
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, 80, seed=2011))
    keys, inv = np.unique(pub, axis=0, return_inverse=True)
    keys, inv = keys.copy(), inv.reshape(-1)
    assert len(keys) == 80
    keys[3, 63] ^= 1                                                                    # off the curve
    keys[7, :32] = np.frombuffer(b32(P + 5), np.uint8)                                  # x >= p: not canonical
    keys[70, 63] ^= 1
    q = keys[TRAP].copy()
    keys[TRAP, 32:] = np.frombuffer(b32(P - _int(q[32:])), np.uint8)                    # -Q: what the trap's signatures are under
    trap_entry = q.copy()
    trap_entry[63] ^= 1                                                                 # what the set lists: (X, Y ^ 1)
    assert not _on_curve(trap_entry) and _on_curve(keys[TRAP]) and (trap_entry[63] & 1) == (keys[TRAP, 63] & 1)
    t = np.nonzero(inv == TRAP)[0]
    dig[t] = TC._rows([(N - _int(x) % N) % N for x in dig[t]])
    s[t] = TC._rows([(N - _int(x)) % N for x in s[t]])
    rng = np.random.default_rng(2012)
    hit = rng.permutation(NSIG)[:NSIG // 10]
    for arr, part in zip((r, s, dig), np.array_split(hit, 3)):
        arr[part, rng.integers(16, 32, size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    flip = np.nonzero((np.arange(NSIG) % 2 == 1) & (inv != TRAP))[0]
    s[flip] = TC._rows([(N - _int(x)) % N for x in s[flip]])
    pub = np.ascontiguousarray(keys[inv])
    point = np.array([_on_curve(k) for k in keys])
    assert not point[[3, 7, 70]].any() and point.sum() == 77
    comp = np.array([bool(point[inv[i]]) and (i % 2 == 0 or inv[i] == TRAP) for i in range(NSIG)])
    pubs = [_compressed(pub[i]) if comp[i] else b"\x04" + bytes(pub[i]) for i in range(NSIG)]
    digs = [bytes(d) for d in dig]
    ders = [_der(r[i], s[i]) for i in range(NSIG)]
    compact = [bytes(r[i]) + bytes(s[i]) for i in range(NSIG)]
    # 40 malformed items on top of well-formed material: a truncated signature, the prefix 05, a 64-byte key, 02 || ff..ff
    bad_pubs, bad_ders, bad_compact = [], [], []
    for j in range(40):
        i = 100 + 7 * j
        k, d, c = pubs[i], ders[i], compact[i]
        if j % 4 == 0:
            d, c = d[:-1], c[:-1]
        elif j % 4 == 1:
            k = b"\x05" + _compressed(pub[i])[1:]
        elif j % 4 == 2:
            k = bytes(pub[i])
        else:
            k = b"\x02" + b"\xff" * 32
        bad_pubs.append(k)
        bad_ders.append(d)
        bad_compact.append(c)
        digs.append(digs[i])
    pubs += bad_pubs
    ders += bad_ders
    compact += bad_compact
    n = NSIG + 40
    wellformed = np.arange(n) < NSIG
    exp = {}
    for rm in (False, True):
        o = oracle.ecdsa_verify_batch(pub, dig, r, s, reject_malleable=rm, nthreads=os.cpu_count() or 1)
        exp[rm] = np.concatenate([o, np.zeros(40, np.uint8)])
    # (encoding, reject_malleable, bip0066) -> (signatures, the oracle's verdicts)
    combos = {("der", False, False): (ders, exp[False]), ("der", True, False): (ders, exp[True]),
              ("compact", False, False): (compact, exp[False]), ("compact", True, False): (compact, exp[True]),
              ("der", False, True): ([d + b"\x01" for d in ders], exp[True])}
    ref = {}
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    try:
        for (enc, rm, b66), (sigs, want) in combos.items():
            got = eng.ecdsa_verify_encoded_batch(pubs, digs, sigs, encoding=S.ENCODING_ASN1 if enc == "der" else S.ENCODING_COMPACT,
                                                 reject_malleable=rm, bip0066=b66)
            assert np.array_equal(got, want), (enc, rm, b66, np.nonzero(got != want)[0][:10])
            ref[(enc, rm, b66)] = got
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
    assert exp[False][t].sum() > 0.8 * len(t), "the trap's signatures verify under -Q"
    for v in ref.values():
        assert 0.3 < v.mean() < 0.9
    other = np.unique(np.array(synth_batch(eng, 64, 64, seed=2013)[0]), axis=0)
    set_keys = keys[:64].copy()
    set_keys[TRAP] = trap_entry
    comp_all = np.concatenate([comp, np.zeros(40, bool)])
    inv_all = np.concatenate([inv, np.full(40, -1)])

    def counts(in_set):
        """(33-byte hits, 65-byte hits, canonical compressed misses) of the well-formed items over a set holding keys[in_set]"""
        held = np.isin(inv_all, in_set) & wellformed
        h33, h65 = int((held & comp_all).sum()), int((held & ~comp_all).sum())
        return h33, h65, int((wellformed & comp_all & ~held).sum())
    main = counts([k for k in range(64) if k != TRAP])
    assert main[2] >= 257 and main[2] > len(t) > 0
    return dict(pubs=pubs, digs=digs, combos={k: v[0] for k, v in combos.items()}, ref=ref, n=n, trap=t,
                sets=[(set_keys, main), (other, counts([])), (keys, counts(list(range(80))))])


def _call(eng, S, ks, c, combo, **kw):
    enc, rm, b66 = combo
    return eng.ecdsa_verify_encoded_batch_keyset(ks, c["pubs"], c["digs"], c["combos"][combo],
                                                 encoding=S.ENCODING_ASN1 if enc == "der" else S.ENCODING_COMPACT,
                                                 reject_malleable=rm, bip0066=b66, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_encoded_keyset_verdicts(eng, enc_case, layout):
    import secp256k1_voi_amd as S
    c = enc_case
    sets = []
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    try:
        for keys, (h33, h65, roots) in c["sets"]:
            ks = eng.keyset_create(keys, getattr(S, layout))
            sets.append(ks)
            ks.index_create()
            for combo, ref in c["ref"].items():
                got = _call(eng, S, ks, c, combo)
                st, ek = eng.key_grouping_stats(), eng.last_encoded_keyset_stats()
                assert np.array_equal(got, ref), (len(keys), combo, np.nonzero(got != ref)[0][:10])
                assert st["keyed"] == h33 + h65 and st["general"] == c["n"] - h33 - h65 and st["tables"] == 0, (len(keys), combo, st)
                assert ek == dict(hits33=h33, hits65=h65, roots=roots, delegated=0), (len(keys), combo, ek)
        # the set with the trap: its signatures came compressed, missed the off-curve entry, and verify after a root
        got = _call(eng, S, sets[0], c, ("der", False, False))
        assert got[c["trap"]].sum() > 0.8 * len(c["trap"])
        assert c["sets"][1][1][:2] == (0, 0) and c["sets"][2][1][2] == 0
        got = _call(eng, S, sets[0], c, ("der", False, False), force_worklist=True)
        assert np.array_equal(got, c["ref"][("der", False, False)])
        # every item that is not decided before the ladder through the worklist kernel: more than either side alone has
        keyed = sum(c["sets"][0][1][:2])
        assert max(keyed, c["n"] - keyed) < eng.key_grouping_stats()["complete"] <= c["n"]
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        for ks in sets:
            ks.close()


# ---- 3. exceptional lanes ----
def test_encoded_exceptional_lanes(eng, oracle):
    """The chosen-scalar batch of test_gpu_keyset_bykey.test_exceptional_lanes_among_hits_and_misses (1024 signatures, 16 keys,
    8 in the set: u1 = 0 and R = identity lanes on both sides), compact-encoded with compressed keys."""
    import secp256k1_voi_amd as S
    n, n_keys = 1024, 16
    rng = random.Random(1921)
    d = [rng.randrange(1, N) for _ in range(n_keys)]
    base = TC.chosen_u2()
    u2 = [base[i % len(base)] for i in range(n)]
    key = [i % n_keys for i in range(n)]
    kind = [0 if i < n // 2 else 1 + ((i // n_keys) & 1) for i in range(n)]            # 0 random u1, 1 u1 = 0, 2 R = identity
    u1 = [rng.randrange(N) if kd == 0 else 0 if kd == 1 else (-b * d[k]) % N for b, k, kd in zip(u2, key, kind)]
    kR = [(a + b * d[k]) % N for a, b, k in zip(u1, u2, key)]
    Rp = eng.scalar_base_mult_batch(TC._rows([v or 1 for v in kR]))
    Q = np.ascontiguousarray(eng.scalar_base_mult_batch(TC._rows(d))[:, 1:])
    rr = [_int(Rp[i, 1:33]) % N if kR[i] else rng.randrange(1, N) for i in range(n)]
    ss = [x * pow(b, -1, N) % N for x, b in zip(rr, u2)]
    ee = [a * x % N for a, x in zip(u1, ss)]
    dig, r, s = TC._rows(ee), TC._rows(rr), TC._rows(ss)
    pub = np.ascontiguousarray(Q[key])
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1)
    kinds = np.array(kind)
    assert 0 < exp.sum() < n and (kinds == 1).sum() >= n // 8
    pubs = [_compressed(k) for k in pub]
    digs = [bytes(x) for x in dig]
    sigs = [bytes(r[i]) + bytes(s[i]) for i in range(n)]
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    sets = []
    try:
        for layout in (S.KEYSET_COMB, S.KEYSET_JOINT5):
            ks = eng.keyset_create(Q[:8], layout)
            sets.append(ks)
            ks.index_create()
            got = eng.ecdsa_verify_encoded_batch_keyset(ks, pubs, digs, sigs, encoding=S.ENCODING_COMPACT)
            assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
            assert eng.key_grouping_stats()["complete"] >= int((kinds == 1).sum()), "the u1 = 0 lanes of both sides are the worklist's"
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        for ks in sets:
            ks.close()


# ---- 4. pieces ----
def test_encoded_keyset_pieces(eng):
    """A synchronous call above three rounds of the ladder goes in pieces of two rounds (a round: 3 * 4 * CUs * 64
    signatures).  n = 2 pieces + 1037: the last piece is below the small-batch threshold, so it is parsed and verified as the
    plain call does and the set is not used for it.  Compact signatures and compressed keys as (blob, offsets) pairs."""
    import torch
    import secp256k1_voi_amd as S
    from secp256k1_voi_amd.synth import synth_batch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rnd = 3 * 4 * cus * 64
    last = 1037
    n = 2 * (2 * rnd) + last
    assert n > 3 * rnd and last <= ROW_DEFAULT
    m = 1024
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, m, 64, seed=2031))
    r[::9, 31] ^= 1                                                                      # a ninth damaged
    idx = np.arange(n) % m
    pk = np.empty((n, 33), np.uint8)
    pk[:, 0] = 2 + (pub[idx, 63] & 1)
    pk[:, 1:] = pub[idx, :32]
    sg = np.concatenate([r[idx], s[idx]], axis=1)
    dg = np.ascontiguousarray(dig[idx])
    args = [(np.ascontiguousarray(a).reshape(-1), np.arange(n + 1, dtype=np.uint64) * w) for a, w in ((pk, 33), (dg, 32), (sg, 64))]
    ks = eng.keyset_create(np.unique(pub, axis=0), S.KEYSET_COMB)
    try:
        ks.index_create()
        ref = eng.ecdsa_verify_encoded_batch_submit(*args, encoding=S.ENCODING_COMPACT).wait()
        got = eng.ecdsa_verify_encoded_batch_keyset(ks, *args, encoding=S.ENCODING_COMPACT)
        ek = eng.last_encoded_keyset_stats()
        assert np.array_equal(got, ref) and 0.8 * n < int(got.sum()) < 0.95 * n
        assert ek == dict(hits33=n - last, hits65=0, roots=0, delegated=last), ek
    finally:
        ks.close()


# ---- 5. delegation, tickets, refusals ----
def test_encoded_keyset_delegation_tickets_refusals(eng, enc_case):
    import ctypes as C
    import secp256k1_voi_amd as S
    c = enc_case
    der, compact = ("der", False, False), ("compact", True, False)
    ks = eng.keyset_create(c["sets"][0][0], S.KEYSET_COMB)
    bare = eng.keyset_create(c["sets"][0][0], S.KEYSET_COMB)
    other_eng = S.Engine(0)
    try:
        ks.index_create()
        # default thresholds: a call of 1000 items IS the plain call (no grouping, no worklist, the set unused)
        m = 1000
        got = eng.ecdsa_verify_encoded_batch_keyset(ks, c["pubs"][:m], c["digs"][:m], c["combos"][der][:m])
        assert eng.key_grouping_stats() == dict(keyed=0, tables=0, general=0, complete=0)
        assert eng.last_encoded_keyset_stats() == dict(hits33=0, hits65=0, roots=0, delegated=m)
        assert np.array_equal(got, c["ref"][der][:m])
        assert np.array_equal(got, eng.ecdsa_verify_encoded_batch(c["pubs"][:m], c["digs"][:m], c["combos"][der][:m]))
        assert eng.ecdsa_verify_encoded_batch_keyset(ks, [], [], []).shape == (0,)
        # two tickets of the submit form in flight beside a plain encoded ticket
        eng.set_small_batch_max(0)
        eng.set_mid_batch_max(0)
        try:
            t1 = eng.ecdsa_verify_encoded_batch_keyset_submit(ks, c["pubs"], c["digs"], c["combos"][der])
            t2 = eng.ecdsa_verify_encoded_batch_submit(c["pubs"], c["digs"], c["combos"][der])
            t3 = eng.ecdsa_verify_encoded_batch_keyset_submit(ks, c["pubs"], c["digs"], c["combos"][compact], encoding=S.ENCODING_COMPACT,
                                                              reject_malleable=True)
            assert np.array_equal(t3.wait(), c["ref"][compact])
            assert np.array_equal(t1.wait(), c["ref"][der]) and np.array_equal(t2.wait(), c["ref"][der])
            assert np.array_equal(_call(eng, S, ks, c, der), c["ref"][der]) and np.array_equal(_call(eng, S, ks, c, compact), c["ref"][compact])
        finally:
            eng.set_small_batch_max(ROW_DEFAULT)
            eng.set_mid_batch_max(QUAD_DEFAULT)
        # refusals
        rec = [x + b"\x00" for x in c["combos"][compact][:m]]
        with pytest.raises(S.EngineError):
            eng.ecdsa_verify_encoded_batch_keyset(ks, c["pubs"][:m], c["digs"][:m], rec, encoding=S.ENCODING_COMPACT_RECOVERABLE)
        with pytest.raises(S.EngineError):
            eng.ecdsa_verify_encoded_batch_keyset_submit(ks, c["pubs"][:m], c["digs"][:m], rec, encoding=S.ENCODING_COMPACT_RECOVERABLE)
        with pytest.raises(S.EngineError):
            eng.ecdsa_verify_encoded_batch_keyset(bare, c["pubs"][:m], c["digs"][:m], c["combos"][der][:m])      # no index
        with pytest.raises(S.EngineError):
            other_eng.ecdsa_verify_encoded_batch_keyset(ks, c["pubs"][:m], c["digs"][:m], c["combos"][der][:m])  # another engine's set
        n_, a, _ = eng._encoded_keyset_args(c["pubs"][:m], c["digs"][:m], c["combos"][der][:m], False, False, False)
        out = np.zeros(n_, np.uint8)
        with pytest.raises(S.EngineError):
            eng._check(eng._lib.s2k_ecdsa_verify_encoded_batch_keyset(eng._h, ks._k, n_, *(x.ctypes.data for x in a), S.ENCODING_ASN1, 0,
                                                                      S.FORCE_COMPLETE, out.ctypes.data))
        tk = C.c_uint64(0)
        with pytest.raises(S.EngineError):
            eng._check(eng._lib.s2k_ecdsa_verify_encoded_batch_keyset_submit(eng._h, ks._k, n_, *(x.ctypes.data for x in a), S.ENCODING_ASN1,
                                                                             0, S.FORCE_COMPLETE, out.ctypes.data, C.byref(tk)))
        with pytest.raises(ValueError):
            eng.ecdsa_verify_encoded_batch_keyset(ks, c["pubs"][:m], c["digs"][:m - 1], c["combos"][der][:m])
    finally:
        other_eng.close()
        bare.close()
        ks.close()
