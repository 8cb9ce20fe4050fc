"""The byte-level model of the parse step (ingest_model.py) pinned on the CPU, so that the GPU tests compare the kernels with
something that is itself checked: against the oracle's restatement of the DER parser and its SEC1 key decoding, against the
host parsers of the library (der.h compiled for the host), against pyref for the square root, and against the oracle's
verdicts - on the whole corpus (ingest_corpus.py), both Wycheproof files and the BIP-0066 vectors."""
import secp256k1_voi_amd as S
import ingest_corpus as C
import ingest_model as M
import pyref as R
from conftest import load_golden

H = bytes.fromhex


def _all_entries():
    for cfg in C.CONFIGS:
        rep, once = C.corpus(cfg)
        for e in rep + once:
            yield (cfg,) + e


def _check_signature_bytes(oracle, sig, where):
    rc, r, s = M.parse_asn1_signature(sig)
    want = (r, s) if rc == 0 else None
    assert oracle.parse_asn1_signature(sig) == want, where
    assert S.parse_asn1_signature(sig) == want, where
    assert S.load_library().s2k_parse_asn1_signature(sig, len(sig), bytes(32), bytes(32)) == rc, where
    rc, r, s = M.parse_compact_signature(sig)
    assert S.parse_compact_signature(sig) == ((r, s) if rc == 0 else None), where
    assert S.load_library().s2k_parse_compact_signature(sig, len(sig), bytes(32), bytes(32)) == rc, where
    assert bool(S.is_valid_signature_encoding_bip0066(sig)) == M.is_valid_signature_encoding_bip0066(sig), where


def test_model_signature_parsers_on_the_corpus(oracle):
    seen = set()
    for cfg, cls, _, _, sig in _all_entries():
        for g in (sig, sig[:-1], sig + b"\x01"):                 # (as it is, without a sighash byte, with one)
            if g not in seen:
                seen.add(g)
                _check_signature_bytes(oracle, g, (cfg, cls, g.hex()))
    assert len(seen) > 500


def test_model_on_wycheproof_and_bip0066(oracle):
    total = accepted = 0
    for fn in ("wycheproof_ecdsa_sha256.json", "wycheproof_ecdsa_sha512.json"):
        for c in load_golden(fn)["cases"]:
            sig, pub, digest = H(c["sig"]), H(c["pub"]), H(c["digest"])
            _check_signature_bytes(oracle, sig, (fn, c["tcId"]))
            it = M.parse_item(pub, digest, sig, M.ASN1)
            total += 1
            accepted += it.ok
            if c["valid"]:
                assert it.ok, (fn, c["tcId"])
            if not it.ok:
                assert not c["valid"] and oracle.ecdsa_verify_asn1(pub, digest, sig) == 0, (fn, c["tcId"])
            else:
                assert it.xy == pub[1:] and it.dg == digest[:32] and (it.r, it.s) == oracle.parse_asn1_signature(sig)
    assert total == 996 and 300 < accepted < total - 100
    d = load_golden("bip0066.json")
    for i, v in enumerate(d["valid"]):
        g = H(v["der"]) + b"\x45"
        assert M.is_valid_signature_encoding_bip0066(g)
        _check_signature_bytes(oracle, g, ("bip0066 valid", i))
        rc, r, s = M.parse_asn1_signature(g[:-1])
        if i == 8:                                                # r = s = 0: the shape is fine, the scalars are not
            assert rc == 2
        else:
            assert rc == 0 and (int.from_bytes(r, "big"), int.from_bytes(s, "big")) == (int(v["r"], 16), int(v["s"], 16))
    for i, v in enumerate(d["invalid_decode"]):
        g = H(v["der"]) + b"\x45"
        assert not M.is_valid_signature_encoding_bip0066(g), v["exception"]
        _check_signature_bytes(oracle, g, ("bip0066 invalid", i))


def test_model_keys_against_oracle_and_pyref(oracle):
    n33 = 0
    for cls, key in C.key_classes():
        xy = M.decode_key(key)
        ref = oracle.point_from_bytes(key)
        if ref == oracle.IDENTITY:                                # (00: a point, and no public key - secec.go:206-209)
            assert key == b"\x00"
            ref = None
        if len(key) == 65 and key[0] == 4:
            # verbatim at this step; the oracle's NewPointFromBytes also checks the coordinates
            assert xy == key[1:]
            assert (ref is not None) == M.set_valid(key[1:]), cls
        else:
            assert (xy is None) == (ref is None), cls
            if xy is not None:
                assert b"\x04" + xy == ref, cls
        if len(key) == 33 and key[0] in (2, 3):
            n33 += 1
            pt = R.lift_x(int.from_bytes(key[1:], "big"), key[0] & 1)
            assert (xy is None) == (pt is None), cls
            if pt is not None:
                assert xy == R.b32(pt[0]) + R.b32(pt[1]) and R.on_curve(pt), cls
    assert n33 >= 15
    for a in (0, 1, 2, 3, 4, 7, R.P - 1, R.P - 2, 5**40):
        assert M.sqrt_p(a) == R.sqrt_p(a) or {M.sqrt_p(a), R.sqrt_p(a)} == {None}
    names = [c for c, _ in C.key_classes()]
    assert len(set(names)) == len(names)
    for want in ("key/02_root_negated", "key/02_root_as_computed", "key/03_root_negated", "key/03_root_as_computed", "key/02_no_root",
                 "key/02_x=p", "key/04_off_curve", "key/04_x>=p", "key/len_0", "key/len_66", "key/prefix_07_65", "key/04_on_33", "key/02_on_65"):
        assert want in names, want


def test_corpus_valid_signatures_verify_and_damage_does_not(oracle):
    valid = C.valid_signatures()
    assert len(valid) == 3 + 8 + 64
    for j, sg in enumerate(valid):
        assert oracle.ecdsa_verify_raw(sg.key[1:], sg.digest, R.b32(sg.r), R.b32(sg.s)), sg.name
        assert oracle.ecdsa_recover(sg.digest, R.b32(sg.r), R.b32(sg.s), sg.v) == sg.key, sg.name
        if j < 3 or j % 9 == 0:                                   # (pyref is slow: the signed ones and a sample of the rest)
            assert R.ecdsa_verify(R.dec65(sg.key), sg.digest, sg.r, sg.s), sg.name
    lens_r = {(sg.r.bit_length() + 7) // 8 for sg in valid}
    lens_s = {(sg.s.bit_length() + 7) // 8 for sg in valid}
    assert lens_r == set(range(1, 33)) and lens_s == set(range(1, 33))
    assert {sg.s for sg in valid} >= {1, R.N - 1, (R.N - 1) // 2, (R.N - 1) // 2 + 1}
    enc, dl, rm, bip = C.CONFIGS["der"]
    rep, _ = C.corpus("der")
    for cls, key, digest, sig in rep:
        it = M.parse_item(key, digest, sig, enc, dl, rm, bip)
        verdict = oracle.ecdsa_verify_asn1(key, digest, sig)
        if cls.startswith("valid/") or cls.endswith("+twin"):
            assert it.ok and verdict == 1, cls
        if cls.startswith(("der/", "sig/raw_len")) and not cls.endswith("+twin"):
            assert not it.ok, cls
        if not it.ok:
            assert verdict in (0, -1), cls                        # (-1: the oracle could not construct the key)
        else:
            assert (it.r, it.s) == oracle.parse_asn1_signature(sig) and it.dg == digest[:32], cls


def test_model_options():
    """the option handling of Verify as the parse step sees it"""
    sg = next(v for v in C.valid_signatures() if v.s == (R.N - 1) // 2 + 1)
    lo = next(v for v in C.valid_signatures() if v.s == (R.N - 1) // 2)
    raw = R.b32(sg.r) + R.b32(sg.s)
    d = sg.digest
    assert M.parse_item(sg.key, d, raw, M.COMPACT, 0, True).ok                      # (the ladder's rule, not the parse step's)
    assert M.parse_item(sg.key, d, raw + b"\x00", M.COMPACT_RECOVERABLE, 0, False).ok
    assert not M.parse_item(sg.key, d, raw + b"\x00", M.COMPACT_RECOVERABLE, 0, True).ok
    assert M.parse_item(lo.key, lo.digest, R.b32(lo.r) + R.b32(lo.s) + b"\x07", M.COMPACT_RECOVERABLE, 0, True).recid == 7
    assert not M.parse_item(sg.key, d + d, raw, M.COMPACT, 32).ok and M.parse_item(sg.key, d + d, raw, M.COMPACT, 64).ok
    assert M.parse_item(sg.key, d + d, raw, M.COMPACT, 0).dg == d and not M.parse_item(sg.key, d[:31], raw, M.COMPACT, 0).ok
    der = C.der_sig(sg.r, sg.s)
    assert M.parse_item(sg.key, d, der + b"\x01", M.ASN1, 0, False, True).ok and not M.parse_item(sg.key, d, der, M.ASN1, 0, False, True).ok
    assert not M.parse_item(sg.key, d + d, der + b"\x01", M.ASN1, 64, False, True).ok  # BIP-0066 implies 32-byte digests
    bad = M.parse_item(b"", d, der, M.ASN1)
    assert (bad.ok, bad.dg, bad.r, bad.s, bad.recid) == (False, bytes(32), bytes(32), bytes(32), 0xFF)


def test_set_model():
    q = C.valid_signatures()[0].key[1:]
    neg = q[:32] + R.b32(R.P - int.from_bytes(q[32:], "big"))
    off = q[:63] + bytes([q[63] ^ 1])                        # off the curve, the parity of -Q
    other = C.valid_signatures()[1].key[1:]
    ks = M.SetModel([off, other, q, q, neg, off])
    assert ks.found64(off) == 0 and ks.found64(q) == 2 and ks.found64(neg) == 4 and ks.found64(bytes(64)) == M.NONE
    cq, cn = bytes([2 + (q[63] & 1)]) + q[:32], bytes([2 + (neg[63] & 1)]) + neg[:32]
    assert ks.found33(cq) == 2 and ks.found33(cn) == 4, "the off-curve entry of -Q's parity is never answered"
    assert ks.found33(b"\x05" + q[:32]) == M.NONE and ks.found33(cq + b"\x00") == M.NONE
    sg = C.valid_signatures()[0]
    sig = C.der_sig(sg.r, sg.s)
    nx = next(k for c, k in C.key_classes() if c == "key/02_no_root")
    big = next(k for c, k in C.key_classes() if c == "key/02_x=p")
    fresh = next(k for c, k in C.key_classes() if c == "key/02_root_negated")
    keys = [cq, b"\x04" + off, b"\x04" + bytes(64), fresh, nx, big, cq, b"\x04" + q]
    sigs = [sig] * 6 + [sig[:-1], sig]
    items, found, counts = M.parse_items_keyset(ks, keys, [sg.digest] * 8, sigs, M.ASN1)
    assert found == [2, 0, M.NONE, M.NONE, M.NONE, M.NONE, M.NONE, 2]
    assert [i.ok for i in items] == [True, True, True, True, False, False, False, True]
    assert counts == dict(hits33=1, hits65=2, roots=2, root_items=[3, 4]) and items[0].xy == q


def test_layout_alignment_and_vacuity():
    """what the GPU test asserts from the offsets before it touches the device, here for every configuration"""
    for cfg, (enc, dl, rm, bip) in C.CONFIGS.items():
        L = C.layout(cfg)
        assert len(L) <= 4096, cfg
        starts = {}
        pos = [0, 0, 0]
        for cls, k, d, g in L:
            for j, b in enumerate((k, d, g)):
                starts.setdefault((cls, j), set()).add(pos[j] % 16)
                pos[j] += len(b)
        rep, _ = C.corpus(cfg)
        for cls in {c for c, *_ in rep}:
            assert starts[(cls, 0)] == set(range(16)) and starts[(cls, 2)] == set(range(16)), (cfg, cls)
        ok = sum(M.parse_item(k, d, g, enc, dl, rm, bip).ok for _, k, d, g in L)
        if cfg == "der":
            assert 4 * ok >= len(L) and 4 * (len(L) - ok) >= len(L)
        assert 10 * ok >= len(L) and 10 * (len(L) - ok) >= len(L), cfg
