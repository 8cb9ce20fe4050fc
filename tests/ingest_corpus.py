"""The corpus of the parse-step tests (test_ingest_model.py on the CPU, test_gpu_ingest_items.py on the device): keys, digests
and encoded signatures, class by class, so that a failure names its class.  Deterministic; no GPU.

An entry is (class name, key bytes, digest bytes, signature bytes).  corpus(config) gives (repeated, once): the entries that
the layout repeats at every alignment, and long runs of same-shaped entries (every value of V, ...) that it lays out once.

Valid signatures: a handful signed with pyref; the others fix (r, s, v, digest) and take the key the oracle RECOVERS, which
makes a valid signature out of any s in [1, n) and any r that is an x coordinate: s = 1, n - 1 and the two values on the low-s
constant, and r / s of every big-endian length from 1 to 32 bytes, the top bit set (a 33-byte DER integer) and clear."""
import functools
import hashlib

import pyref as R

P, N = R.P, R.N
HALF = (N - 1) // 2
ASN1, COMPACT, RECOVERABLE = 0, 1, 2
b32 = R.b32

# name -> (encoding, digest_len, reject_malleable, bip0066)
CONFIGS = {
    "der": (ASN1, 0, False, False),
    "der_len32": (ASN1, 32, False, False),
    "der_len64": (ASN1, 64, True, False),
    "bip0066": (ASN1, 0, False, True),
    "compact": (COMPACT, 0, False, False),
    "compact_low_s": (COMPACT, 32, True, False),
    "recoverable": (RECOVERABLE, 0, False, False),
    "recoverable_low_s": (RECOVERABLE, 0, True, False),
}


def _oracle():
    import oracle as O
    O.build()
    return O


def _h(tag, n=32):
    out = b""
    i = 0
    while len(out) < n:
        out += hashlib.sha256(b"ingest corpus|%s|%d" % (tag.encode(), i)).digest()
        i += 1
    return out[:n]


def _x_on_curve_from(x):
    while R.lift_x(x, 0) is None:
        x += 1
    return x


def _with_length(nbytes, top_bit, tag):
    """a value of exactly nbytes big-endian bytes, its top bit as asked"""
    v = int.from_bytes(_h(tag, nbytes), "big")
    v &= (1 << (8 * nbytes - 1)) - 1
    if top_bit:
        v |= 1 << (8 * nbytes - 1)
    else:
        v |= 1 << (8 * nbytes - 2) if nbytes > 1 or v == 0 else 0
        v &= (1 << (8 * nbytes - 1)) - 1
        v |= 1 if v == 0 else 0
    assert (v.bit_length() + 7) // 8 == nbytes and bool(v >> (8 * nbytes - 1)) == bool(top_bit)
    return v


class Sig:
    """a VALID signature: (r, s, v) on `digest` under `key` (65 bytes, 04 || X || Y)"""

    def __init__(self, name, r, s, v, digest, key):
        self.name, self.r, self.s, self.v, self.digest, self.key = name, r, s, v, digest, key


def _recovered(name, r, s, v=0, digest=None):
    digest = digest if digest is not None else _h("digest|" + name)
    key = _oracle().ecdsa_recover(digest, b32(r), b32(s), v)
    assert key is not None, name
    return Sig(name, r, s, v, digest, key)


@functools.lru_cache(maxsize=None)
def valid_signatures():
    out = []
    # signed, not recovered: private key d, nonce k
    for j in range(3):
        d, k = int.from_bytes(_h("d%d" % j), "big") % N or 1, int.from_bytes(_h("k%d" % j), "big") % N or 1
        digest = _h("signed%d" % j, 32 + 16 * j)
        r, s = R.ecdsa_sign(d, digest, k)
        Rp, Q = R.mul(k, R.G), R.mul(d, R.G)
        v = (Rp[1] & 1) | (2 if Rp[0] >= N else 0)
        out.append(Sig("valid/signed%d" % j, r, s, v, digest, R.enc65(Q)))
    rx = _x_on_curve_from((1 << 255) + int.from_bytes(_h("r", 24), "big"))          # (the top bit set: 33 bytes in DER)
    for name, s in (("s=1", 1), ("s=n-1", N - 1), ("s=half", HALF), ("s=half+1", HALF + 1)):
        for v in (0, 1):
            out.append(_recovered("valid/%s/v%d" % (name, v), rx, s, v))
    sx = int.from_bytes(_h("s"), "big") % HALF
    for nbytes in range(1, 33):
        top = nbytes & 1
        lo = 1 << (8 * nbytes - 1) if top else max(1, 1 << (8 * nbytes - 2)) if nbytes > 1 else 1
        r = _x_on_curve_from(lo if nbytes < 32 else _with_length(32, top, "r32") % N if not top else (1 << 255) + 12345)
        assert (r.bit_length() + 7) // 8 == nbytes and r < N and bool(r >> (8 * nbytes - 1)) == bool(top)
        out.append(_recovered("valid/r_len%d_top%d" % (nbytes, top), r, sx, nbytes & 1))
        s = _with_length(nbytes, 1 - top, "slen%d" % nbytes)
        if s >= N:
            s = (1 << 255) + 98765
        out.append(_recovered("valid/s_len%d_top%d" % (nbytes, 1 - top), rx, s, 0))
    return tuple(out)


# ---- DER ----
def der_len(n):
    if n < 128:
        return bytes([n])
    b = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(b)]) + b


def der_int_bytes(v):
    return v.to_bytes(v.bit_length() // 8 + 1, "big")           # minimal, with the zero in front of a set top bit


def tlv(tag, body):
    return bytes([tag]) + der_len(len(body)) + body


def der_sig(r, s):
    return tlv(0x30, tlv(0x02, der_int_bytes(r)) + tlv(0x02, der_int_bytes(s)))


def der_damage(r, s):
    """(class, bytes) for every way a lenient parser would forgive; r and s: a valid signature's"""
    ri, si = der_int_bytes(r), der_int_bytes(s)
    R_, S_ = tlv(2, ri), tlv(2, si)
    body = R_ + S_
    good = tlv(0x30, body)
    n = len(body)
    out = [
        ("long_form_81_seq", b"\x30\x81" + bytes([n]) + body),
        ("long_form_81_int", tlv(0x30, b"\x02\x81" + bytes([len(ri)]) + ri + S_)),
        ("len_82_leading_zero", b"\x30\x82\x00" + bytes([n]) + body),
        ("len_83_leading_zero", b"\x30\x83\x00\x00" + bytes([n]) + body),
        ("len_84_leading_zero", b"\x30\x84\x00\x00\x00" + bytes([n]) + body),
        ("len_85", b"\x30\x85\x00\x00\x00\x00" + bytes([n]) + body),
        ("indefinite_80", b"\x30\x80" + body + b"\x00\x00"),
        ("redundant_00_r", tlv(0x30, tlv(2, b"\x00" + ri) + S_)),
        ("redundant_00_s", tlv(0x30, R_ + tlv(2, b"\x00" + si))),
        ("redundant_ff_r", tlv(0x30, tlv(2, b"\xff" + bytes([ri[0] | 0x80]) + ri[1:]) + S_)),
        ("redundant_ff_s", tlv(0x30, R_ + tlv(2, b"\xff" + bytes([si[0] | 0x80]) + si[1:]))),
        ("negative_r", tlv(0x30, tlv(2, (b32(r | 1 << 255))) + S_)),
        ("negative_s", tlv(0x30, R_ + tlv(2, (b32(s | 1 << 255))))),
        ("empty_integer_r", tlv(0x30, b"\x02\x00" + S_)),
        ("empty_integer_s", tlv(0x30, R_ + b"\x02\x00")),
        ("tag_31", b"\x31" + good[1:]),
        ("tag_03_r", tlv(0x30, b"\x03" + R_[1:] + S_)),
        ("tag_03_s", tlv(0x30, R_ + b"\x03" + S_[1:])),
        ("tag_1f", b"\x1f" + good[1:]),
        ("tag_3f", b"\x3f" + good[1:]),
        ("tag_1f_r", tlv(0x30, b"\x1f" + R_[1:] + S_)),
        ("trailing_inside", tlv(0x30, body + b"\x00")),
        ("trailing_inside_tlv", tlv(0x30, body + b"\x02\x01\x01")),
        ("trailing_behind", good + b"\x00"),
        ("trailing_behind_2", good + b"\x05\x00"),
        ("seq_len_short", b"\x30" + bytes([n - 1]) + body),
        ("seq_len_long", b"\x30" + bytes([n + 1]) + body),
        ("empty", b""),
        ("one_byte", b"\x30"),
        ("int_34_bytes_r", tlv(0x30, tlv(2, b"\x00\x80" + b32(r)) + S_)),
        ("int_34_bytes_s", tlv(0x30, R_ + tlv(2, b"\x01\x00" + b32(s)))),
        ("int_33_bytes_no_zero", tlv(0x30, tlv(2, b"\x01" + b32(r)) + S_)),
    ]
    for name, v in (("0", 0), ("n", N), ("n+1", N + 1), ("2^256-1", 2**256 - 1)):
        out.append(("r=" + name, der_sig(v, s)))
        out.append(("s=" + name, der_sig(r, v)))
    return out


def truncations(good):
    return [("truncated", good[:k]) for k in range(len(good))]


# ---- keys ----
def _compressed(key65, prefix=None):
    return bytes([prefix if prefix is not None else 2 + (key65[64] & 1)]) + key65[1:33]


@functools.lru_cache(maxsize=None)
def key_classes():
    """(class, key bytes); the first entry of each valid kind decodes to the key of a valid signature"""
    base = valid_signatures()[0].key
    out = [("key/04", base)]
    # 02 / 03 where the root the power (p + 1) / 4 gives has the asked parity, and where it is its negation
    want = {(p, flip) for p in (2, 3) for flip in (0, 1)}
    x = int.from_bytes(_h("kx"), "big") % P
    while want:
        x = _x_on_curve_from(x + 1)
        y0 = pow((x * x * x + 7) % P, (P + 1) // 4, P)
        for p in (2, 3):
            flip = int((y0 & 1) != (p & 1))
            if (p, flip) in want:
                want.discard((p, flip))
                out.append(("key/0%d_root_%s" % (p, "negated" if flip else "as_computed"), bytes([p]) + b32(x)))
                break
    out.append(("key/compressed_of_valid", _compressed(base)))
    nx = int.from_bytes(_h("noroot"), "big") % P
    while R.lift_x(nx, 0) is not None:
        nx += 1
    out.append(("key/02_no_root", b"\x02" + b32(nx)))
    out.append(("key/03_no_root", b"\x03" + b32(nx)))
    for name, v in (("0", 0), ("p-1", P - 1), ("p", P), ("p+1", P + 1), ("2^256-1", 2**256 - 1)):
        out.append(("key/02_x=" + name, b"\x02" + b32(v)))
        out.append(("key/03_x=" + name, b"\x03" + b32(v)))
    for p in (0x00, 0x05, 0x06, 0x07):
        out.append(("key/prefix_%02x_33" % p, bytes([p]) + base[1:33]))
        out.append(("key/prefix_%02x_65" % p, bytes([p]) + base[1:]))
    out.append(("key/04_on_33", b"\x04" + base[1:33]))
    out.append(("key/02_on_65", b"\x02" + base[1:]))
    out.append(("key/03_on_65", b"\x03" + base[1:]))
    for n in (0, 1, 32, 34, 64, 66):
        out.append(("key/len_%d" % n, (base + b"\x01")[:n] if n != 1 else b"\x00"))
    off = bytearray(base)
    off[64] ^= 1
    out.append(("key/04_off_curve", bytes(off)))
    out.append(("key/04_x>=p", b"\x04" + b32(P + 3) + base[33:]))
    out.append(("key/04_y>=p", b"\x04" + base[1:33] + b32(2**256 - 1)))
    return tuple(out)


def digest_classes():
    return [("digest/len_%d" % n, _h("dlen%d" % n, n)) for n in (0, 31, 32, 33, 64, 200)]


# ---- the corpus of a configuration ----
def _encode(sg, encoding, bip0066):
    if encoding == ASN1:
        return der_sig(sg.r, sg.s) + (b"\x01" if bip0066 else b"")
    raw = b32(sg.r) + b32(sg.s)
    return raw if encoding == COMPACT else raw + bytes([sg.v])


def _digest_for(sg, digest_len):
    """the signature's digest at the configuration's length: the leftmost 32 bytes are what was signed"""
    want = digest_len or len(sg.digest)
    return (sg.digest + _h("pad|" + sg.name, 200))[:max(want, 32)] if want >= len(sg.digest) else sg.digest[:max(want, 32)]


@functools.lru_cache(maxsize=None)
def corpus(config):
    import json
    import os
    encoding, digest_len, low_s, bip = CONFIGS[config]
    valid = valid_signatures()
    rep, once = [], []

    def emit(dst, cls, key, digest, sig):
        dst.append((cls, bytes(key), bytes(digest), bytes(sig)))

    def twin(dst, sg, cls):
        emit(dst, cls + "+twin", sg.key, _digest_for(sg, digest_len), _encode(sg, encoding, bip))

    if bip:        # (the vectors and edges of the shape check take the room: r and s of the extreme lengths only)
        valid = tuple(v for v in valid if "_len" not in v.name or v.name.split("_len")[1].split("_")[0] in ("1", "2", "31", "32"))
    for sg in valid:
        emit(rep, sg.name, sg.key, _digest_for(sg, digest_len), _encode(sg, encoding, bip))
    base = valid[3]
    assert base.name.startswith("valid/s=1")
    hi = next(v for v in valid if v.name.startswith("valid/s=n-1"))          # both integers of 33 bytes when r's top bit is set too
    sh = b"\x01" if bip else b""
    if encoding == ASN1:
        for cls, bad in der_damage(hi.r, hi.s):
            emit(rep, "der/" + cls, hi.key, _digest_for(hi, digest_len), bad + sh)
        twin(rep, hi, "der/damage")
        for cls, bad in truncations(_encode(hi, encoding, bip)):
            emit(rep, "der/" + cls, hi.key, _digest_for(hi, digest_len), bad)
        twin(rep, hi, "der/truncated")
    if bip:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bip0066.json")) as f:
            vec = json.load(f)
        for kind in ("valid", "invalid_decode"):
            for j, v in enumerate(vec[kind]):
                emit(rep, "bip0066/json_%s_%d" % (kind, j), base.key, _digest_for(base, 32), bytes.fromhex(v["der"]) + b"\x45")
        # total lengths 8, 9, 73 and 74 with the sighash byte: the shortest and the longest strings the shape check takes, and
        # one byte beyond either
        big = (1 << 255) + 5
        edge = [("len9_r=1_s=1", der_sig(1, 1)), ("len8_empty_s", tlv(0x30, tlv(2, b"\x01") + b"\x02\x00")),
                ("len8_truncated", der_sig(1, 1)[:-1]), ("len73_both_33", der_sig(big, big + 2)),
                ("len74_redundant_00", tlv(0x30, tlv(2, b"\x00" + der_int_bytes(big)) + tlv(2, der_int_bytes(big)))),
                ("len74_trailing", der_sig(big, big + 2) + b"\x00"), ("len73_long_form", b"\x30\x81\x45" + der_sig(big, big)[2:-1]),
                ("len9_negative", tlv(0x30, tlv(2, b"\x80") + tlv(2, b"\x01"))), ("len10_r=0x80", der_sig(0x80, 1))]
        for cls, g in edge:
            emit(rep, "bip0066/" + cls, base.key, _digest_for(base, 32), g + b"\x01")
            assert cls.startswith("len%d_" % (len(g) + 1)), (cls, len(g) + 1)
        emit(rep, "bip0066/no_sighash_byte", base.key, _digest_for(base, 32), der_sig(base.r, base.s))
        twin(rep, base, "bip0066/edges")
    # strings of the lengths around the two compact forms, under every encoding
    raw = b32(base.r) + b32(base.s) + bytes([base.v]) + b"\x00"
    for n in (0, 63, 64, 65, 66):
        emit(rep, "sig/raw_len_%d" % n, base.key, _digest_for(base, digest_len), raw[:n])
    if encoding != ASN1:
        tail = b"" if encoding == COMPACT else b"\x00"
        for name, v in (("0", 0), ("n", N), ("n+1", N + 1), ("2^256-1", 2**256 - 1)):
            emit(rep, "compact/r=" + name, base.key, _digest_for(base, digest_len), b32(v) + b32(base.s) + tail)
            emit(rep, "compact/s=" + name, base.key, _digest_for(base, digest_len), b32(base.r) + b32(v) + tail)
        twin(rep, base, "compact/range")
    if encoding == RECOVERABLE:
        for v in range(256):
            emit(once, "recoverable/V=every_byte", base.key, _digest_for(base, digest_len), b32(base.r) + b32(base.s) + bytes([v]))
    # keys: under a signature that is valid for the first of them
    k0 = valid[0]
    for cls, key in key_classes():
        emit(rep, cls, key, _digest_for(k0, digest_len), _encode(k0, encoding, bip))
    for cls, d in digest_classes():
        emit(rep, cls, k0.key, d, _encode(k0, encoding, bip))
    return tuple(rep), tuple(once)


# ---- layout ----
def layout(config, reps=16):
    """The corpus laid out `reps` times, a spacer item in front of each repetition whose three strings have the 0 .. 15 bytes
    that make the repetition start at residue k mod 16 in every blob; the `once` entries follow.  Returns the entries
    [(class, key, digest, sig)] with the spacers as class "spacer"."""
    rep, once = corpus(config)
    out = []
    pos = [0, 0, 0]
    for k in range(reps):
        sp = [bytes((k - p) % 16) for p in pos]
        out.append(("spacer", sp[0], sp[1], sp[2]))
        out.extend(rep)
        for j in range(3):
            pos[j] += len(sp[j]) + sum(len(e[1 + j]) for e in rep)
    out.extend(once)
    return out
