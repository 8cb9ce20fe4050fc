"""The accept rule of every verification ladder, on near misses that keep R fixed (tests/accept_corpus.py).

Every kernel ends in a comparison of x(R) with r - Jacobian X == r Z^2 on 9 x 29 limbs, homogeneous X == r Z in the row field,
affine x after a shared inversion -, for ECDSA a second one with r + n under r < p - n, for BIP-340 the parity of y(R).  The
corpus holds, next to valid signatures, items whose u1 and u2 are those of a valid one and whose r differs from x(R) in one
bit (every bit), by n in either direction, or only in the parity of y: the ladder ends in the same point and nothing but that
last step can tell them apart.  tests/test_accept_corpus_cpu.py has shown that the oracle stands behind every expected value
and which classes a sloppy comparison would let through.

Each case sends the WHOLE batch down one route, compares the whole output with the oracle's, and checks through
key_grouping_stats / last_keyed_ladder / last_keyset_ladder that the route was the one it meant."""
import contextlib

import numpy as np
import pytest

import accept_corpus as A
from conftest import load_golden

pytestmark = pytest.mark.gpu
N = A.N
ZERO = {"keyed": 0, "tables": 0, "general": 0, "complete": 0}
LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]
ROW_LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT5"]
SMALL_DEFAULT, MID_DEFAULT, KS_SMALL_DEFAULT = 3072, 32768, 2048        # what a new context starts with (engine_internal.h)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(oracle):
    return A.corpus(oracle)


@contextlib.contextmanager
def route(eng, small=SMALL_DEFAULT, mid=MID_DEFAULT, ks_small=KS_SMALL_DEFAULT, grouping=None, min_group=0, ladder=None):
    """the context's thresholds and grouping for one call; a new context's settings afterwards"""
    import secp256k1_voi_amd as S
    try:
        eng.set_small_batch_max(small)
        eng.set_mid_batch_max(mid)
        eng.set_keyset_small_batch_max(ks_small)
        eng.set_key_grouping(S.KEYS_ADAPTIVE if grouping is None else grouping, min_group=min_group)
        eng.set_keyed_ladder(S.LADDER_COMB if ladder is None else ladder)
        yield
    finally:
        eng.set_small_batch_max(SMALL_DEFAULT)
        eng.set_mid_batch_max(MID_DEFAULT)
        eng.set_keyset_small_batch_max(KS_SMALL_DEFAULT)
        eng.set_key_grouping(S.KEYS_ADAPTIVE)
        eng.set_keyed_ladder(S.LADDER_COMB)


def same(got, exp, cls):
    diffs, count = A.first_differences(got, exp, cls)
    assert count == 0, f"{count} of {len(exp)} differ; the first (index, class, got, expected): {diffs}"


def in_range(ec):
    """items whose r and s pass the range check: the lanes that reach a ladder"""
    ints = lambda a: [int.from_bytes(bytes(v), "big") for v in a]
    return sum(0 < r < N and 0 < s < N for r, s in zip(ints(ec["r"]), ints(ec["s"])))


# ---- ECDSA ---------------------------------------------------------------------------------------------------------------
def _ecdsa(eng, ec, **kw):
    return eng.ecdsa_verify_batch(ec["pub"], ec["dig"], ec["r"], ec["s"], **kw)


def test_ecdsa_wave_per_signature(eng, corpus):
    """k_verify_row: X == r Z in the row field"""
    ec = corpus["ecdsa"]
    with route(eng, small=4096):
        got, st = _ecdsa(eng, ec), eng.key_grouping_stats()
    same(got, ec["exp"], ec["cls"])
    assert st == ZERO, st


def test_ecdsa_four_lanes_per_signature(eng, corpus):
    """k_verify_quad"""
    ec = corpus["ecdsa"]
    with route(eng, small=0, mid=32768):
        got, st = _ecdsa(eng, ec), eng.key_grouping_stats()
    same(got, ec["exp"], ec["cls"])
    assert st == ZERO, st


def test_ecdsa_lane_per_signature(eng, corpus):
    """k_verify_fast, MODE_ECDSA: Jacobian X == r Z^2.  With the grouping off nothing is counted (`general` counts what a
    grouping left over: the next case); the worklist stays empty, so every verdict is this kernel's."""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    with route(eng, small=0, mid=0, grouping=S.KEYS_OFF):
        got, st, last = _ecdsa(eng, ec), eng.key_grouping_stats(), eng.last_keyed_ladder()
    same(got, ec["exp"], ec["cls"])
    assert st == ZERO and last == -1, (st, last)


def test_ecdsa_lane_per_signature_left(eng, corpus):
    """MODE_ECDSA_LEFT: a grouping whose threshold no key reaches leaves every signature to the general ladder"""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    n = len(ec["cls"])
    with route(eng, small=0, mid=0, grouping=S.KEYS_AUTO, min_group=4096):
        got, st = _ecdsa(eng, ec), eng.key_grouping_stats()
    same(got, ec["exp"], ec["cls"])
    assert st == {"keyed": 0, "tables": 0, "general": n, "complete": 0}, st


def test_ecdsa_force_complete(eng, corpus):
    """k_ecdsa_verify: the complete path in every lane"""
    ec = corpus["ecdsa"]
    with route(eng):
        got, st = _ecdsa(eng, ec, force_complete=True), eng.key_grouping_stats()
    same(got, ec["exp"], ec["cls"])
    assert st == ZERO, st


def test_ecdsa_force_worklist(eng, corpus):
    """k_verify_fallback: every lane that reaches the ladder is handed to the worklist kernel"""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    with route(eng, grouping=S.KEYS_OFF):
        got, st = _ecdsa(eng, ec, force_worklist=True), eng.key_grouping_stats()
    same(got, ec["exp"], ec["cls"])
    assert st == {"keyed": 0, "tables": 0, "general": 0, "complete": in_range(ec)}, st


@pytest.mark.parametrize("ladder", ["comb", "window"])
def test_ecdsa_grouped(eng, corpus, ladder):
    """S2K_KEYS_ALWAYS: a table for each of the eight keys, MODE_ECDSA_COMB / MODE_ECDSA_KEYED for every signature"""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    want = S.LADDER_COMB if ladder == "comb" else S.LADDER_WINDOW
    with route(eng, small=0, mid=0, grouping=S.KEYS_ALWAYS, ladder=want):
        got, st, last = _ecdsa(eng, ec), eng.key_grouping_stats(), eng.last_keyed_ladder()
    same(got, ec["exp"], ec["cls"])
    assert last == want
    assert st == {"keyed": len(ec["cls"]), "tables": len(ec["keys"]), "general": 0, "complete": 0}, st


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ecdsa_keyset_lane(eng, corpus, layout):
    """every corpus key in a set of each layout, the lane-per-signature ladder over its tables"""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    ks = eng.keyset_create(ec["keys"], getattr(S, layout))
    try:
        assert ks.layout() == getattr(S, layout) and ks.valid_keys().all()
        with route(eng, ks_small=0):
            got = eng.ecdsa_verify_batch_keyset(ks, ec["kidx"], ec["dig"], ec["r"], ec["s"])
            last, st = eng.last_keyset_ladder(), eng.key_grouping_stats()
    finally:
        ks.close()
    same(got, ec["exp"], ec["cls"])
    assert last == S.KEYSET_LADDER_LANE and st["complete"] == 0, (last, st)


def test_ecdsa_keyset_force_worklist(eng, corpus):
    """k_verify_fallback_keyset"""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    ks = eng.keyset_create(ec["keys"], S.KEYSET_JOINT)
    try:
        with route(eng):
            got = eng.ecdsa_verify_batch_keyset(ks, ec["kidx"], ec["dig"], ec["r"], ec["s"], force_worklist=True)
            last, st = eng.last_keyset_ladder(), eng.key_grouping_stats()
    finally:
        ks.close()
    same(got, ec["exp"], ec["cls"])
    assert last == S.KEYSET_LADDER_LANE and st["complete"] == in_range(ec), (last, st)


@pytest.mark.parametrize("layout", ROW_LAYOUTS)
def test_ecdsa_keyset_row(eng, corpus, layout):
    """k_verify_row_keyset"""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    ks = eng.keyset_create(ec["keys"], getattr(S, layout))
    try:
        with route(eng, ks_small=4096):
            got = eng.ecdsa_verify_batch_keyset(ks, ec["kidx"], ec["dig"], ec["r"], ec["s"])
            last, st = eng.last_keyset_ladder(), eng.key_grouping_stats()
    finally:
        ks.close()
    same(got, ec["exp"], ec["cls"])
    assert last == S.KEYSET_LADDER_ROW and st == ZERO, (last, st)


# ---- BIP-340 -------------------------------------------------------------------------------------------------------------
def _schnorr(eng, bip, **kw):
    return eng.schnorr_verify_batch(bip["pk32"], bip["msgs"], bip["sig"], **kw)


def test_schnorr_wave_per_signature(eng, corpus):
    """k_schnorr_row"""
    bip = corpus["schnorr"]
    with route(eng, small=4096):
        got, st = _schnorr(eng, bip), eng.key_grouping_stats()
    same(got, bip["exp"], bip["cls"])
    assert st == ZERO, st


def test_schnorr_four_lanes_per_signature(eng, corpus):
    """k_schnorr_quad"""
    bip = corpus["schnorr"]
    with route(eng, small=0, mid=32768):
        got, st = _schnorr(eng, bip), eng.key_grouping_stats()
    same(got, bip["exp"], bip["cls"])
    assert st == ZERO, st


def test_schnorr_lane_per_signature(eng, corpus):
    """k_verify_fast, MODE_SCHNORR, then k_affine_finish: the affine x and the parity of y"""
    import secp256k1_voi_amd as S
    bip = corpus["schnorr"]
    with route(eng, small=0, mid=0, grouping=S.KEYS_OFF):
        got, st, last = _schnorr(eng, bip), eng.key_grouping_stats(), eng.last_keyed_ladder()
    same(got, bip["exp"], bip["cls"])
    assert (st["keyed"], st["tables"], st["general"]) == (0, 0, 0) and last == -1, (st, last)


def test_schnorr_lane_per_signature_left(eng, corpus):
    """MODE_SCHNORR_LEFT: a grouping that leaves every signature to the general ladder"""
    import secp256k1_voi_amd as S
    bip = corpus["schnorr"]
    with route(eng, small=0, mid=0, grouping=S.KEYS_AUTO, min_group=4096):
        got, st = _schnorr(eng, bip), eng.key_grouping_stats()
    same(got, bip["exp"], bip["cls"])
    assert (st["keyed"], st["tables"], st["general"]) == (0, 0, len(bip["cls"])), st


def test_schnorr_force_complete(eng, corpus):
    """the complete path in every lane (a call that reports nothing about its route)"""
    bip = corpus["schnorr"]
    with route(eng):
        got = _schnorr(eng, bip, force_complete=True)
    same(got, bip["exp"], bip["cls"])


@pytest.mark.parametrize("ladder", ["comb", "window"])
def test_schnorr_grouped(eng, corpus, ladder):
    """S2K_KEYS_ALWAYS: MODE_SCHNORR_COMB / MODE_SCHNORR_KEYED on the three keys' tables"""
    import secp256k1_voi_amd as S
    bip = corpus["schnorr"]
    want = S.LADDER_COMB if ladder == "comb" else S.LADDER_WINDOW
    with route(eng, small=0, mid=0, grouping=S.KEYS_ALWAYS, ladder=want):
        got, st, last = _schnorr(eng, bip), eng.key_grouping_stats(), eng.last_keyed_ladder()
    same(got, bip["exp"], bip["cls"])
    assert last == want
    assert (st["keyed"], st["tables"], st["general"]) == (len(bip["cls"]), len(bip["keys"]), 0), st


@pytest.mark.parametrize("layout", LAYOUTS)
def test_schnorr_keyset_lane(eng, corpus, layout):
    """key 1 of the set is stored with odd Y"""
    import secp256k1_voi_amd as S
    bip = corpus["schnorr"]
    ks = eng.keyset_create(bip["keys"], getattr(S, layout))
    try:
        assert ks.layout() == getattr(S, layout) and ks.valid_keys().all()
        with route(eng, ks_small=0):
            got = eng.schnorr_verify_batch_keyset(ks, bip["kidx"], bip["msgs"], bip["sig"])
            last = eng.last_keyset_ladder()
    finally:
        ks.close()
    same(got, bip["exp"], bip["cls"])
    assert last == S.KEYSET_LADDER_LANE


@pytest.mark.parametrize("layout", ROW_LAYOUTS)
def test_schnorr_keyset_row(eng, corpus, layout):
    """k_schnorr_row_keyset"""
    import secp256k1_voi_amd as S
    bip = corpus["schnorr"]
    ks = eng.keyset_create(bip["keys"], getattr(S, layout))
    try:
        with route(eng, ks_small=4096):
            got = eng.schnorr_verify_batch_keyset(ks, bip["kidx"], bip["msgs"], bip["sig"])
            last, st = eng.last_keyset_ladder(), eng.key_grouping_stats()
    finally:
        ks.close()
    same(got, bip["exp"], bip["cls"])
    assert last == S.KEYSET_LADDER_ROW and st == ZERO, (last, st)


# ---- recovery ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["wave", "quad", "lane", "complete"])
def test_recovery(eng, corpus, path):
    """every valid ECDSA item with its id gives 04 || Q (bit 1 of the id set for the wrapped ones); a wrapped r without
    bit 1 or with the other parity gives what the oracle finds there; an ordinary r with bit 1 (r + n >= p) gives nothing"""
    rec = corpus["recovery"]
    small, mid = {"wave": (4096, MID_DEFAULT), "quad": (0, 32768), "lane": (0, 0), "complete": (SMALL_DEFAULT, MID_DEFAULT)}[path]
    with route(eng, small=small, mid=mid):
        pub65, ok = eng.ecdsa_recover_batch(rec["dig"], rec["r"], rec["s"], rec["rid"], force_complete=path == "complete")
    same(ok, rec["exp_ok"], rec["cls"])
    same((pub65 != rec["exp_pub"]).any(axis=1), np.zeros(len(ok), bool), rec["cls"])


# ---- the device's BIP-0066 shape check (ingest.hip: pe_item) on input that is not well-formed -----------------------------------
def _der_int(v):
    b = v.to_bytes((v.bit_length() + 8) // 8 or 1, "big")
    return b"\x02" + bytes([len(b)]) + b


def _der_variants(r, s):
    """(name, signature without the sighash byte): well-formed, one per rule of IsValidSignatureEncoding broken, and one
    that passes the shape rules with an r that is no scalar"""
    ri, si = _der_int(r), _der_int(s)
    seq = lambda body, tag=0x30, extra=0: bytes([tag, len(body) + extra]) + body
    big = r + N if r + N < 2**256 else N
    # negative: the high bit of the first content byte set (or the 00 in front of such a byte dropped); padded: a 00 too many
    neg = lambda b: b"\x02" + bytes([b[1] - 1]) + b[3:] if b[2] == 0 and b[1] > 1 else b[:2] + bytes([b[2] | 0x80]) + b[3:]
    pad = lambda b: b"\x02" + bytes([b[1] + 1]) + b"\x00" + b[2:]
    longer = lambda b: b[:1] + bytes([b[1] + 1]) + b[2:]
    return [("well_formed", seq(ri + si)),
            ("total_length_long", seq(ri + si, extra=1)), ("total_length_short", seq(ri + si, extra=-1)),
            ("r_length", seq(longer(ri) + si)), ("s_length", seq(ri + longer(si))),
            ("r_empty", seq(b"\x02\x00" + si)), ("s_empty", seq(ri + b"\x02\x00")),
            ("r_negative", seq(neg(ri) + si)), ("s_negative", seq(ri + neg(si))),
            ("r_padded", seq(pad(ri) + si)), ("s_padded", seq(ri + pad(si))),
            ("sequence_tag", seq(ri + si, tag=0x31)), ("r_tag", seq(b"\x03" + ri[1:] + si)), ("s_tag", seq(ri + b"\x03" + si[1:])),
            ("r_not_a_scalar", seq(_der_int(big) + si))]


def test_bip0066_shapes_on_the_device(eng, corpus, oracle):
    """bitcoin.VerifyASN1 on the device: 24 valid corpus signatures, each well-formed, with each shape rule broken and with
    r >= n in a well-formed shape; then the negative vectors of the BIP.  Expected: the host's shape check (which passes the
    golden vectors, test_host_parsing.py), then the oracle's parser and its low-s verification."""
    import secp256k1_voi_amd as S
    ec = corpus["ecdsa"]
    pick = np.nonzero(ec["exp"] == 1)[0][:24]
    pubs, digs, sigs, names, exp = [], [], [], [], []
    for i in pick:
        q, dg = bytes(ec["pub"][i]), bytes(ec["dig"][i])
        for name, der in _der_variants(int.from_bytes(bytes(ec["r"][i]), "big"), int.from_bytes(bytes(ec["s"][i]), "big")):
            sig = der + b"\x01"
            rs = oracle.parse_asn1_signature(der)
            shape = S.is_valid_signature_encoding_bip0066(sig)
            assert shape == (name in ("well_formed", "r_not_a_scalar")), (name, sig.hex())
            assert (rs is not None) == (name == "well_formed"), (name, sig.hex())
            pubs.append(b"\x04" + q), digs.append(dg), sigs.append(sig), names.append(name)
            exp.append(int(shape and rs is not None and oracle.ecdsa_verify_raw(q, dg, rs[0], rs[1], True)))
    well = [e for e, name in zip(exp, names) if name == "well_formed"]
    assert 0 < sum(well) < len(well) and sum(exp) == sum(well)           # low s accepted, high s not; nothing else
    q, dg = bytes(ec["pub"][pick[0]]), bytes(ec["dig"][pick[0]])
    for v in load_golden("bip0066.json")["invalid_decode"]:
        pubs.append(b"\x04" + q), digs.append(dg), sigs.append(bytes.fromhex(v["der"]) + b"\x01"), names.append("vector: " + v["exception"])
        exp.append(0)
    got = eng.ecdsa_verify_encoded_batch(pubs, digs, sigs, bip0066=True)
    same(got, np.array(exp, np.uint8), names)
