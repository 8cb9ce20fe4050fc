"""The device parse step of the encoded ECDSA calls, item by item: k_parse_encoded, k_parse_encoded_keyset, k_decompress_list
and k_decompress_list_close run through s2k_debug_parse_encoded (the product's own launch helpers, no ladder behind them) and
compared byte for byte with the model of ingest_model.py on the corpus of ingest_corpus.py.

For every item of the piece: the model says ok -> xy, digest, r, s (and the recovery id) are the model's bytes; the model says
not ok -> digest = r = s = 0 and the recovery id is 0xff (xy of a failed item is not part of the contract).  Rows outside the
piece still hold the sentinel the hook filled the arrays with.  No tolerance anywhere."""
import numpy as np
import pytest

import ingest_corpus as C
import ingest_model as M
import pyref as R

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


# ---- helpers ----
def blobs(entries, first_offsets=(0, 0, 0)):
    """three (blob, offsets) pairs; first_offsets: bytes of filler in front of each blob, which the offsets skip"""
    out = []
    for j in range(3):
        strings = [e[1 + j] for e in entries]
        offs = np.zeros(len(strings) + 1, dtype=np.uint64)
        offs[0] = first_offsets[j]
        offs[1:] = first_offsets[j] + np.cumsum([len(x) for x in strings], dtype=np.uint64)
        blob = np.frombuffer(b"\xEE" * first_offsets[j] + b"".join(strings) + b"\0", dtype=np.uint8)[:-1]
        if blob.size == 0:
            blob = np.zeros(1, np.uint8)
        out.append((np.ascontiguousarray(blob), offs))
    return out


def model_items(entries, cfg):
    enc, dl, rm, bip = C.CONFIGS[cfg]
    return [M.parse_item(k, d, g, enc, dl, rm, bip) for _, k, d, g in entries]


def run(eng, entries, cfg, first=0, cnt=None, first_offsets=(0, 0, 0), **kw):
    enc, dl, rm, bip = C.CONFIGS[cfg]
    b = blobs(entries, first_offsets)
    return eng.debug_parse_encoded(b[0], b[1], b[2], first=first, cnt=cnt, encoding=enc, digest_len=dl, reject_malleable=rm, bip0066=bip,
                                   sentinel=SENTINEL, **kw)


def _rows(strings, width):
    return np.frombuffer(b"".join(strings), np.uint8).reshape(len(strings), width)


def check(out, entries, items, first, cnt, recoverable):
    """the contract of the parse step on the arrays the hook returned; names the class of the first item that breaks it"""
    n = len(entries)
    inside = np.zeros(n, bool)
    inside[first:first + cnt] = True
    for name in ("xy", "dg", "r", "s"):
        assert (out[name][~inside] == SENTINEL).all(), "%s: a row outside the piece was written: item %d" % (
            name, np.nonzero((out[name] != SENTINEL).any(axis=1) & ~inside)[0][0])
    if recoverable:
        assert (out["recid"][~inside] == SENTINEL).all()
    ok = np.array([it.ok for it in items])
    zero64 = bytes(64)
    exp = dict(xy=_rows([it.xy if it.ok else zero64 for it in items], 64), dg=_rows([it.dg for it in items], 32),
               r=_rows([it.r for it in items], 32), s=_rows([it.s for it in items], 32))
    for name in ("dg", "r", "s", "xy"):
        rows = inside & ok if name == "xy" else inside
        bad = np.nonzero((out[name] != exp[name]).any(axis=1) & rows)[0]
        assert bad.size == 0, "%s of item %d (class %s, model ok = %s): got %s, the model has %s" % (
            name, bad[0], entries[bad[0]][0], ok[bad[0]], bytes(out[name][bad[0]]).hex(), bytes(exp[name][bad[0]]).hex())
    if recoverable:
        want = np.array([it.recid for it in items], np.uint8)
        bad = np.nonzero((out["recid"] != want) & inside)[0]
        assert bad.size == 0, "recid of item %d (class %s): got %#x, the model has %#x" % (bad[0], entries[bad[0]][0], out["recid"][bad[0]], want[bad[0]])


def residues(entries, first_offsets=(0, 0, 0)):
    """(class, blob) -> the residues mod 16 at which an item of the class starts in that blob, from the offsets alone"""
    starts = {}
    b = blobs(entries, first_offsets)
    for j in range(3):
        offs = b[j][1]
        for i, e in enumerate(entries):
            starts.setdefault((e[0], j), set()).add(int(offs[i]) % 16)
    return starts


# ---- 1. the corpus, every class at every alignment ----
@pytest.mark.parametrize("cfg", list(C.CONFIGS))
def test_corpus_items_at_every_alignment(eng, cfg):
    entries = C.layout(cfg)
    n = len(entries)
    assert n <= 4096
    starts = residues(entries)
    for cls in {e[0] for e in C.corpus(cfg)[0]}:
        assert starts[(cls, 0)] == set(range(16)), ("key blob", cls)
        assert starts[(cls, 2)] == set(range(16)), ("signature blob", cls)
    items = model_items(entries, cfg)
    n_ok = sum(it.ok for it in items)
    if cfg == "der":
        # the vacuity guard of the main batch, from the model alone: a quarter of the items ok, a quarter not
        assert 4 * n_ok >= n and 4 * (n - n_ok) >= n
    assert 10 * n_ok >= n and 10 * (n - n_ok) >= n
    out = run(eng, entries, cfg)
    check(out, entries, items, 0, n, C.CONFIGS[cfg][0] == C.RECOVERABLE)


# ---- 2. counts and pieces ----
@pytest.fixture(scope="module")
def piece_case():
    entries = C.layout("der")[:1300]
    return entries, model_items(entries, "der")


@pytest.mark.parametrize("first_offsets", [(0, 0, 0), (37, 5, 1003)])
def test_counts_and_pieces(eng, piece_case, first_offsets):
    entries, items = piece_case
    for first in (0, 1, 255, 256, 257):
        for cnt in (1, 63, 64, 65, 255, 256, 257, 1000):
            out = run(eng, entries, "der", first, cnt, first_offsets)
            try:
                check(out, entries, items, first, cnt, False)
            except AssertionError as e:
                raise AssertionError("first %d, cnt %d: %s" % (first, cnt, e)) from None


def test_pieces_of_the_recoverable_form(eng):
    entries = C.layout("recoverable_low_s", reps=2)
    items = model_items(entries, "recoverable_low_s")
    for first, cnt in ((0, 1), (255, 2), (1, 256), (130, 300)):
        check(run(eng, entries, "recoverable_low_s", first, cnt, (3, 0, 9)), entries, items, first, cnt, True)


# ---- 3. the staging boundary ----
def _ordinary(n):
    """n valid items with signatures of full length (r and s of 31 or 32 bytes)"""
    v = [x for x in C.valid_signatures() if x.r.bit_length() > 240 and x.s.bit_length() > 240]
    assert len(v) >= 8
    return [("ordinary/" + v[i % len(v)].name, v[i % len(v)].key, v[i % len(v)].digest[:32], C.der_sig(v[i % len(v)].r, v[i % len(v)].s))
            for i in range(n)]


@pytest.mark.parametrize("blob", [0, 1, 2])
def test_staging_boundary(eng, blob):
    """One workgroup: 255 ordinary items and, in the middle, one over-long invalid string in one blob, sized so that the
    workgroup's stretch of that blob lands on the fit boundary of the LDS staging, one byte under it and one byte over it.  The
    kernel stages when (hi - (lo & ~15)) + 16 <= capacity.  Whichever side a case falls on, every other item comes out as in
    the run where everything is staged (the long string replaced by an empty one), and as the model has it."""
    import secp256k1_voi_amd as S
    cap = S.parse_encoded_caps()[blob]
    # whatever the capacity is: whole 16-byte loads fill it, and a workgroup of the longest valid strings (65-byte keys,
    # SHA-512 digests, 73-byte signatures) is staged at any alignment - 15 bytes in front of it, 16 behind
    assert cap % 16 == 0 and cap >= 256 * (65, 64, 73)[blob] + 15 + 16
    cfg = "der_len32"                                        # (a digest of another length than 32 is invalid there)
    first_offsets = [0, 0, 0]
    first_offsets[blob] = 21                                 # lo & ~15 = 16: 5 bytes ride in front of the stretch
    base = _ordinary(256)
    mid = 128

    def with_mid(string):
        e = list(base)
        parts = list(e[mid])
        parts[0] = "long"
        parts[1 + blob] = string
        e[mid] = tuple(parts)
        return e
    plain = with_mid(b"")
    items_plain = model_items(plain, cfg)
    assert not items_plain[mid].ok and sum(it.ok for it in items_plain) == 255
    ref = run(eng, plain, cfg, first_offsets=tuple(first_offsets))
    check(ref, plain, items_plain, 0, 256, False)
    lo = first_offsets[blob]
    others = sum(len(e[1 + blob]) for e in plain)
    sides = []
    for delta in (-1, 0, 1, None):
        # (hi - (lo & ~15)) + 16 == cap + delta; None: the extreme, one string of 5 000 bytes
        length = 5000 if delta is None else cap + delta - 16 + (lo & ~15) - lo - others
        assert length > 80                                       # (longer than any valid key, digest or signature)
        e = with_mid(bytes((7 * i + 1) & 0xFF for i in range(length)))
        hi = lo + others + length
        staged = (hi - (lo & ~15)) + 16 <= cap
        sides.append(staged)
        if delta is not None:
            assert (hi - (lo & ~15)) + 16 == cap + delta
        items = model_items(e, cfg)
        assert not items[mid].ok
        out = run(eng, e, cfg, first_offsets=tuple(first_offsets))
        check(out, e, items, 0, 256, False)
        keep = np.arange(256) != mid
        for name in ("xy", "dg", "r", "s"):
            assert np.array_equal(out[name][keep], ref[name][keep]), (name, delta, staged)
    assert sides[:3] == [True, True, False], "one byte under and ON the boundary are staged, one byte over is not"
    assert sides[3] == (blob == 1)       # the 5 000-byte string: far over for keys and signatures; beside 255 digests of 32 bytes it fits


# ---- 4. over a key set ----
def _x_list(tag, count, want_root):
    out, x = [], int.from_bytes(C._h(tag), "big") % R.P
    while len(out) < count:
        x += 1
        if (R.lift_x(x, 0) is not None) == want_root:
            out.append(x)
    return out


@pytest.fixture(scope="module")
def keyset_case():
    """A set of 40 entries: 16 keys, a duplicate of some, negations (both parities of Y under one X), an entry off the curve whose
    parity names the point the set does not hold, and one with X >= p.  The batch, by workgroup of 256:
      0  every lane goes on the list (compressed keys outside the set; every 5th X has no root)
      1  none does (keys of the set, compressed and uncompressed; uncompressed keys outside it; failed items)
      2  exactly one per wave, at lanes 0, 64 + 63, 128 + 17, 192 + 40
      3  mixed, and the piece ends 70 items into it: the second wave is partial, the last two have no item at all"""
    v = C.valid_signatures()
    pts = [R.mul(int.from_bytes(C._h("set%d" % j), "big") % R.N, R.G) for j in range(16)]
    ent = [R.b32(p[0]) + R.b32(p[1]) for p in pts]
    neg = [R.b32(p[0]) + R.b32(R.P - p[1]) for p in pts[:6]]
    off = ent[7][:63] + bytes([ent[7][63] ^ 1])                  # X of key 7 with the parity of -Q7, off the curve
    big = R.b32(R.P + 9) + ent[8][32:]
    entries_set = [off] + ent[:8] + neg[:3] + ent[:4] + [big] + ent[8:] + neg[3:] + [off, ent[15]]
    entries_set += [ent[j % 16] for j in range(40 - len(entries_set))]
    assert len(entries_set) == 40
    ks = M.SetModel(entries_set)
    sig = [C.der_sig(s.r, s.s) for s in v]
    roots_x = _x_list("outside", 300, True)
    noroot_x = _x_list("outside-none", 80, False)

    def comp(e):
        return bytes([2 + (e[63] & 1)]) + e[:32]
    held = [comp(e) for e in ent + neg] + [b"\x04" + e for e in ent + neg + [off, big]]
    batch = []

    def put(cls, key, j, good=True):
        s = v[j % len(v)]
        batch.append((cls, key, s.digest[:32], sig[j % len(v)] if good else sig[j % len(v)][:-1]))
    for j in range(256):
        put("ks/root" if j % 5 else "ks/no_root", bytes([2 + (j & 1)]) + R.b32(roots_x[j] if j % 5 else noroot_x[j // 5]), j)
    for j in range(256):
        kind = j % 4
        if kind < 2:
            put("ks/held", held[(j * 7) % len(held)], j)
        elif kind == 2:
            put("ks/04_outside", v[j % len(v)].key, j)
        else:
            put("ks/failed_signature", comp(R.b32(roots_x[j]) + bytes(32)), j, good=False)
    ones = {0, 64 + 63, 128 + 17, 192 + 40}
    for j in range(256):
        if j in ones:
            put("ks/root_alone_in_wave", b"\x03" + R.b32(roots_x[260 + len(batch) % 30]), j)
        else:
            put("ks/held", held[(j * 5) % len(held)], j)
    trap = comp(off)                 # names the VALID point of X7 with that parity, -Q7: not the set's entry, so it goes on the list
    for j in range(70):
        kind = j % 7
        key = (held[j % len(held)], trap, bytes([3]) + R.b32(roots_x[j]), bytes([2]) + R.b32(noroot_x[j]), b"\x02" + R.b32(R.P + j),
               b"\x04" + off, b"\x05" + ent[0][:32])[kind]
        put("ks/mixed_%d" % kind, key, j, good=(j % 11 != 10))
    return entries_set, ks, batch


def check_keyset(out, batch, ks, first, cnt, roots_before=0):
    piece = batch[first:first + cnt]
    items, found, counts = M.parse_items_keyset(ks, [e[1] for e in piece], [e[2] for e in piece], [e[3] for e in piece], M.ASN1)
    full = [M.Item(False)] * first + items + [M.Item(False)] * (len(batch) - first - cnt)
    check(out, batch, full, first, cnt, False)
    got = out["found"]
    bad = np.nonzero(got != np.array(found, np.uint32))[0]
    assert bad.size == 0, "found[] of item %d (class %s): got %#x, the model has %#x" % (first + bad[0], piece[bad[0]][0], got[bad[0]], found[bad[0]])
    assert out["before"] == dict(hits33=counts["hits33"], hits65=counts["hits65"], roots=roots_before, list=counts["roots"]), out["before"]
    assert out["after"] == dict(hits33=counts["hits33"], hits65=counts["hits65"], roots=roots_before + counts["roots"], list=0), out["after"]
    assert sorted(int(i) for i in out["list"]) == [first + i for i in counts["root_items"]], "the decompression list holds each such item once"
    return counts


def test_keyset_variant(eng, keyset_case):
    import secp256k1_voi_amd as S
    entries_set, ks_model, batch = keyset_case
    n = len(batch)
    assert n == 3 * 256 + 70
    ks = eng.keyset_create(np.frombuffer(b"".join(entries_set), np.uint8).reshape(-1, 64), S.KEYSET_JOINT5)
    try:
        ks.index_create()
        assert [bool(x) for x in ks.valid_keys()] == [M.set_valid(e) for e in entries_set]
        out = run(eng, batch, "der", 0, n, keyset=ks)
        counts = check_keyset(out, batch, ks_model, 0, n)
        # the workgroups are what the docstring of the case says, by the model
        per_wg = [[i for i in counts["root_items"] if 256 * w <= i < 256 * (w + 1)] for w in range(4)]
        assert len(per_wg[0]) == 256 and per_wg[1] == [] and [i - 512 for i in per_wg[2]] == [0, 127, 145, 232]
        assert per_wg[3] and max(per_wg[3]) >= 768 + 64 and counts["hits33"] > 100 and counts["hits65"] > 100
        no_root = [i for i in counts["root_items"] if batch[i][0] in ("ks/no_root", "ks/mixed_3")]
        assert len(no_root) > 50 and (out["r"][no_root] == 0).all() and (out["r"][per_wg[2]] != 0).any(axis=1).all()
        # two pieces of one call, one after the other: the roots add up, the list is empty after each close
        a = run(eng, batch, "der", 0, 256 + 64 + 1, keyset=ks)
        ca = check_keyset(a, batch, ks_model, 0, 256 + 64 + 1)
        b = run(eng, batch, "der", 256 + 64 + 1, n - (256 + 64 + 1), keyset=ks, new_call=False)
        for name in ("hits33", "hits65"):                        # (the counters of a call go on counting)
            b["before"][name] -= ca[name]
            b["after"][name] -= ca[name]
        cb = check_keyset(b, batch, ks_model, 256 + 64 + 1, n - (256 + 64 + 1), roots_before=ca["roots"])
        assert ca["roots"] + cb["roots"] == counts["roots"] and ca["roots"] > 0 and cb["roots"] > 0
        # a piece that ends inside a wave, and one of a single item
        for first, cnt in ((5, 1), (500, 13), (768, 70), (700, 138)):
            check_keyset(run(eng, batch, "der", first, cnt, keyset=ks), batch, ks_model, first, cnt)
    finally:
        ks.close()


@pytest.mark.parametrize("cfg", ["der", "bip0066", "compact_low_s"])
def test_keyset_variant_on_the_corpus(eng, cfg):
    """the corpus through k_parse_encoded_keyset, over a set that holds the keys of half of its valid signatures"""
    import secp256k1_voi_amd as S
    entries = C.layout(cfg, reps=3)
    v = C.valid_signatures()
    entries_set = [s.key[1:] for s in v[::2]]
    off = bytearray(v[1].key[1:])
    off[63] ^= 1
    entries_set = [bytes(off)] + entries_set + [entries_set[0]]
    ks_model = M.SetModel(entries_set)
    enc, dl, rm, bip = C.CONFIGS[cfg]
    items, found, counts = M.parse_items_keyset(ks_model, [e[1] for e in entries], [e[2] for e in entries], [e[3] for e in entries], enc, dl, rm, bip)
    assert counts["hits65"] > 15 and counts["hits33"] >= 3 and counts["roots"] > 10
    ks = eng.keyset_create(np.frombuffer(b"".join(entries_set), np.uint8).reshape(-1, 64), S.KEYSET_COMB if cfg == "der" else S.KEYSET_JOINT5)
    try:
        ks.index_create()
        out = run(eng, entries, cfg, keyset=ks)
        check(out, entries, items, 0, len(entries), False)
        assert np.array_equal(out["found"], np.array(found, np.uint32))
        assert out["after"] == dict(hits33=counts["hits33"], hits65=counts["hits65"], roots=counts["roots"], list=0)
    finally:
        ks.close()


# ---- 5. the low-s constant decides a verdict ----
def test_recoverable_low_s_verdicts(eng):
    """s = (n - 1) / 2 and (n - 1) / 2 + 1, valid recoverable signatures under the key they recover: both verify without
    reject_malleable, the second one does not with it"""
    import secp256k1_voi_amd as S
    half = (R.N - 1) // 2
    sel = [s for s in C.valid_signatures() if s.s in (half, half + 1)]
    assert [s.s - half for s in sel] == [0, 0, 1, 1]
    pubs = [s.key for s in sel]
    digs = [s.digest for s in sel]
    sigs = [R.b32(s.r) + R.b32(s.s) + bytes([s.v]) for s in sel]
    got = eng.ecdsa_verify_encoded_batch(pubs, digs, sigs, encoding=S.ENCODING_COMPACT_RECOVERABLE, reject_malleable=False)
    assert list(got) == [1, 1, 1, 1]
    got = eng.ecdsa_verify_encoded_batch(pubs, digs, sigs, encoding=S.ENCODING_COMPACT_RECOVERABLE, reject_malleable=True)
    assert list(got) == [1, 1, 0, 0]


def test_hook_refuses_what_it_must(eng):
    import secp256k1_voi_amd as S
    entries = _ordinary(8)
    with pytest.raises(S.EngineError):
        run(eng, entries, "der", 4, 5)                               # the piece ends behind the batch
    with pytest.raises(S.EngineError):
        run(eng, entries, "der", 0, 0)
    b = blobs(entries)
    b[2][1][3], b[2][1][4] = b[2][1][4], b[2][1][3]                  # (the hook scans its offsets; the encoded calls do not)
    with pytest.raises(S.EngineError):
        eng.debug_parse_encoded(b[0], b[1], b[2])
