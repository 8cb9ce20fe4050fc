"""A byte-level model of the parse step of the encoded ECDSA calls (k_parse_encoded, k_parse_encoded_keyset,
k_decompress_list), in Python integers and byte strings only.  Written from the rules the reference applies before its
verification runs, as csrc/der.h and csrc/ingest.hip cite them - NOT from the kernels, and importing nothing of the library:

  cryptobyte String.ReadASN1 / ReadASN1Integer (golang.org/x/crypto v0.11.0)      read_asn1, read_asn1_integer
  bytesToCanonicalScalar + the callers' IsZero test (secec/s11n.go:203-218)       canonical_nonzero_scalar
  ParseASN1Signature (s11n.go:83-108)                                             parse_asn1_signature
  ParseCompactSignature / ParseCompactRecoverableSignature (s11n.go:129-168)      parse_compact_signature, parse_recoverable
  IsValidSignatureEncodingBIP0066 (secec/bitcoin/asn1_shitcoin.go:13-115)         is_valid_signature_encoding_bip0066
  PublicKey.Verify's option handling (secec/ecdsa.go:171-228)                     parse_item
  NewPublicKey's length / prefix dispatch, SetCompressedBytes (secec.go:188-216,  decode_key
    point_s11n.go:140-176, :215-230)

What the parse step owes per item (parse_item): `ok`, and for an ok item the exact 64 bytes of the key, 32 of the digest, 32
of r, 32 of s and the recovery id.  An item that is not ok leaves the step with digest = r = s = 0 and recovery id 0xff; its
key bytes are not part of the contract.  A 65-byte 04 key is ok AT THIS STEP whatever its coordinates: the ladder checks that
they are canonical and on the curve, the bytes pass through verbatim."""

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
HALF_N = (N - 1) // 2
ASN1, COMPACT, COMPACT_RECOVERABLE = 0, 1, 2
NONE = 0xFFFFFFFF
ZERO32 = bytes(32)


# ---- cryptobyte ----
def read_asn1(s: bytes, tag: int):
    """String.ReadASN1(&out, tag): (contents, rest) or None.  DER lengths only: the short form below 128, the long form of one
    to four octets with no leading zero octet and a value of at least 128; high-tag-number identifiers are not supported."""
    if len(s) < 2:
        return None
    t, lb = s[0], s[1]
    if t & 0x1F == 0x1F:
        return None
    if lb & 0x80 == 0:
        hdr, length = 2, lb
    else:
        ll = lb & 0x7F
        if ll == 0 or ll > 4 or len(s) < 2 + ll:
            return None
        length = int.from_bytes(s[2:2 + ll], "big")
        if length < 128:
            return None
        if length >> ((ll - 1) * 8) == 0:
            return None
        hdr = 2 + ll
    if len(s) < hdr + length:
        return None
    if t != tag:
        return None
    return s[hdr:hdr + length], s[hdr + length:]


def read_asn1_integer(s: bytes):
    """String.ReadASN1Integer(*[]byte): (magnitude bytes without leading zeros, rest) or None.  The integer is not empty, is
    minimally encoded (no 00 before a byte below 0x80, no ff before a byte from 0x80) and is not negative."""
    got = read_asn1(s, 0x02)
    if got is None:
        return None
    b, rest = got
    if len(b) == 0:
        return None
    if len(b) > 1 and ((b[0] == 0x00 and b[1] & 0x80 == 0) or (b[0] == 0xFF and b[1] & 0x80 == 0x80)):
        return None
    if b[0] & 0x80:
        return None
    while len(b) > 1 and b[0] == 0:
        b = b[1:]
    return b, rest


def canonical_nonzero_scalar(b: bytes):
    """bytesToCanonicalScalar and the IsZero test: the 32-byte big-endian form of a value in [1, n), or None"""
    if len(b) == 0 or len(b) > 32:
        return None
    v = int.from_bytes(b, "big")
    if not 0 < v < N:
        return None
    return v.to_bytes(32, "big")


def parse_asn1_signature(sig: bytes):
    """(rc, r32, s32): rc 0 ok, 1 malformed (errInvalidAsn1Sig), 2 a scalar out of range or zero (errInvalidScalar)"""
    outer = read_asn1(sig, 0x30)
    if outer is None or len(outer[1]) != 0:
        return 1, None, None
    a = read_asn1_integer(outer[0])
    if a is None:
        return 1, None, None
    b = read_asn1_integer(a[1])
    if b is None or len(b[1]) != 0:
        return 1, None, None
    r, s = canonical_nonzero_scalar(a[0]), canonical_nonzero_scalar(b[0])
    if r is None or s is None:
        return 2, None, None
    return 0, r, s


def parse_compact_signature(sig: bytes):
    if len(sig) != 64:
        return 1, None, None
    r, s = canonical_nonzero_scalar(sig[:32]), canonical_nonzero_scalar(sig[32:])
    if r is None or s is None:
        return 2, None, None
    return 0, r, s


def parse_recoverable(sig: bytes):
    """(rc, r32, s32, v): [R | S | V], 65 bytes; V is handed on as it is (RecoverPublicKey judges it)"""
    if len(sig) != 65:
        return 1, None, None, None
    rc, r, s = parse_compact_signature(sig[:64])
    return rc, r, s, (sig[64] if rc == 0 else None)


def is_valid_signature_encoding_bip0066(sig: bytes) -> bool:
    """BIP-0066's IsValidSignatureEncoding on the signature WITH its sighash byte"""
    n = len(sig)
    if n < 9 or n > 73:
        return False
    if sig[0] != 0x30:
        return False
    if sig[1] != n - 3:
        return False
    len_r = sig[3]
    if 5 + len_r >= n:
        return False
    len_s = sig[5 + len_r]
    if len_r + len_s + 7 != n:
        return False
    if sig[2] != 0x02:
        return False
    if len_r == 0:
        return False
    if sig[4] & 0x80:
        return False
    if len_r > 1 and sig[4] == 0x00 and not sig[5] & 0x80:
        return False
    if sig[len_r + 4] != 0x02:
        return False
    if len_s == 0:
        return False
    if sig[len_r + 6] & 0x80:
        return False
    if len_s > 1 and sig[len_r + 6] == 0x00 and not sig[len_r + 7] & 0x80:
        return False
    return True


# ---- keys ----
def sqrt_p(a: int):
    """a square root of a mod p (p = 3 mod 4), or None"""
    r = pow(a, (P + 1) // 4, P)
    return r if r * r % P == a % P else None


def decode_key(key: bytes):
    """NewPublicKey as far as the parse step goes: the 64 bytes X || Y, or None.  65 bytes with prefix 04: the bytes verbatim
    (coordinates and curve equation are the ladder's to check).  33 bytes with prefix 02 / 03: SetCompressedBytes - X below p,
    X^3 + 7 a square, Y the root of the asked parity.  Everything else (other lengths and prefixes, the one-byte identity)
    is no public key."""
    if len(key) == 65 and key[0] == 0x04:
        return bytes(key[1:])
    if len(key) == 33 and key[0] in (0x02, 0x03):
        x = int.from_bytes(key[1:], "big")
        if x >= P:
            return None
        y = sqrt_p((x * x * x + 7) % P)
        if y is None:
            return None
        if (y & 1) != (key[0] & 1):
            y = P - y
        return key[1:] + y.to_bytes(32, "big")
    return None


# ---- an item ----
def parse_signature(digest: bytes, sig: bytes, encoding: int, digest_len: int = 0, reject_malleable: bool = False, bip0066: bool = False):
    """Everything of PublicKey.Verify before the key is looked at: (digest32, r32, s32, v) or None.
    digest_len 0 is opts == nil: any digest of at least 32 bytes (hashToScalar refuses shorter ones), the leftmost 32 used;
    otherwise the digest has exactly that length.  bip0066 (bitcoin.VerifyASN1): the shape check on the signature with its
    sighash byte, which is then dropped; 32-byte digests; low s.  The low-s rule itself is not applied here: see
    low_s_at_parse."""
    if bip0066:
        digest_len, reject_malleable = 32, True
    if digest_len and len(digest) != digest_len:
        return None
    if len(digest) < 32:
        return None
    if bip0066:
        if encoding != ASN1 or not is_valid_signature_encoding_bip0066(sig):
            return None
        sig = sig[:-1]
    v = 0
    if encoding == ASN1:
        rc, r, s = parse_asn1_signature(sig)
    elif encoding == COMPACT:
        rc, r, s = parse_compact_signature(sig)
    elif encoding == COMPACT_RECOVERABLE:
        rc, r, s, v = parse_recoverable(sig)
    else:
        return None
    if rc != 0:
        return None
    return bytes(digest[:32]), r, s, v


class Item:
    __slots__ = ("ok", "xy", "dg", "r", "s", "recid")

    def __init__(self, ok, xy=None, dg=ZERO32, r=ZERO32, s=ZERO32, recid=0xFF):
        self.ok, self.xy, self.dg, self.r, self.s, self.recid = ok, xy, dg, r, s, recid


def low_s_at_parse(encoding: int, reject_malleable: bool, bip0066: bool) -> bool:
    """Where the low-s rule is applied.  The ASN.1 and compact encodings hand (r, s) to a verification that takes the rule as
    an option, so the parse step lets a high s through; the recovery path takes no options, so for the recoverable encoding
    the rule is the parse step's."""
    return encoding == COMPACT_RECOVERABLE and reject_malleable        # (BIP-0066 is an option of the ASN.1 encoding alone)


def parse_front(digest, sig, encoding, digest_len=0, reject_malleable=False, bip0066=False):
    """digest and signature as the parse step judges them, before it looks at the key: (digest32, r32, s32, v) or None"""
    got = parse_signature(digest, sig, encoding, digest_len, reject_malleable, bip0066)
    if got is not None and low_s_at_parse(encoding, reject_malleable, bip0066) and int.from_bytes(got[2], "big") > HALF_N:
        return None
    return got


def parse_item(key: bytes, digest: bytes, sig: bytes, encoding: int, digest_len: int = 0, reject_malleable: bool = False,
               bip0066: bool = False) -> Item:
    """What the parse step leaves for one item (k_parse_encoded)"""
    got = parse_front(digest, sig, encoding, digest_len, reject_malleable, bip0066)
    if got is None:
        return Item(False)
    dg, r, s, v = got
    xy = decode_key(key)
    if xy is None:
        return Item(False)
    return Item(True, xy, dg, r, s, v)


# ---- over a key set ----
def set_valid(entry: bytes) -> bool:
    """a key of the set that is a public key: canonical coordinates on the curve (s2k_keyset_valid_keys)"""
    x, y = int.from_bytes(entry[:32], "big"), int.from_bytes(entry[32:], "big")
    return x < P and y < P and (y * y - x * x * x - 7) % P == 0


class SetModel:
    """The set as its index answers.  65-byte keys: the LOWEST index of an entry with these 64 bytes, valid or not.  33-byte
    keys (the header's rule for key_bytes 33): the lowest index of a VALID entry with this X and a Y of the asked parity."""

    def __init__(self, entries):
        self.entries = [bytes(e) for e in entries]
        self.by64, self.by33 = {}, {}
        for i, e in enumerate(self.entries):
            self.by64.setdefault(e, i)
            if set_valid(e):
                self.by33.setdefault((e[63] & 1, e[:32]), i)

    def found64(self, xy: bytes) -> int:
        return self.by64.get(bytes(xy), NONE)

    def found33(self, key: bytes) -> int:
        if len(key) != 33 or key[0] not in (2, 3):
            return NONE
        return self.by33.get((key[0] & 1, bytes(key[1:])), NONE)


def parse_items_keyset(ks: SetModel, keys, digests, sigs, encoding, digest_len=0, reject_malleable=False, bip0066=False):
    """k_parse_encoded_keyset + k_decompress_list for a piece: (items, found, counts).  found[i]: the key's index in the set,
    NONE when the set does not hold it and for every item whose digest or signature failed.  A compressed key the set holds
    decodes to the set's own 64 bytes.  counts: items under a key of the set that came as 33 bytes, as 65 bytes, and the items
    of the decompression list - compressed keys with an X below p that the set does not hold, whether X^3 + 7 has a root
    (the item is ok) or not (it fails like any other)."""
    items, found = [], []
    hits33 = hits65 = roots = 0
    root_items = []
    for i, (k, d, g) in enumerate(zip(keys, digests, sigs)):
        it = parse_item(k, d, g, encoding, digest_len, reject_malleable, bip0066)
        f = NONE
        if parse_front(d, g, encoding, digest_len, reject_malleable, bip0066) is not None:
            if len(k) == 65 and k[0] == 0x04:
                f = ks.found64(k[1:])
                hits65 += f != NONE
            elif len(k) == 33 and k[0] in (2, 3):
                f = ks.found33(k)
                if f != NONE:
                    hits33 += 1
                    assert it.ok and it.xy == ks.entries[f]       # (a valid entry of this X and parity IS the decoded point)
                elif int.from_bytes(k[1:], "big") < P:
                    roots += 1
                    root_items.append(i)
        items.append(it)
        found.append(f)
    return items, found, dict(hits33=hits33, hits65=hits65, roots=roots, root_items=root_items)
