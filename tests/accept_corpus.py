"""Signatures that differ from an accepted one in the LAST step of verification only (the comparison of x(R) with r, the
second comparison with r + n, the parity of y(R) for BIP-340) - for tests/test_gpu_accept_rule.py and its CPU counterpart.

A signature damaged after it was made (a bit of r, of s, of the digest) changes u2 = r / s, so the verifier's ladder ends in
an unrelated point and ANY comparison rejects it.  Here the point comes first: u1, u2 and the key Q are chosen, R = u1 G + u2 Q
is computed once, and every candidate r' on that R gets s = r' / u2 and e = u1 s.  The verifier then recomputes e / s = u1 and
r' / s = u2, reaches exactly R, and the verdict rests on how it compares x(R) with r' alone.

Point arithmetic is the C oracle's (oracle/); scalars are Python integers mod n.  Expected verdicts and recovered keys are
the oracle's.  Everything is seeded: two calls build the same batches."""
import hashlib
import random
import time

import numpy as np

P = 2**256 - 2**32 - 977
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141

# ---- ECDSA classes
ORD_VALID, ORD_BIT = "ord_valid", "ord_bit"          # n > x(R), ordinary: r' = x; r' = x ^ (1 << b), b in 0..255
ORD_MINUS_N = "ord_minus_n"                          # r' = (x - n) mod 2^256: r' + n = x in 256-bit words; r' >= p - n
ORD_MINUS_N_MODP = "ord_minus_n_modp"                # r' = x + p - n: r' + n = x in the field; r' >= p - n
PLUS_N = "plus_n"                                    # r' = x + n where that fits 256 bits: out of range
WRAP_VALID, WRAP_TWIN, WRAP_BIT = "wrap_valid", "wrap_twin", "wrap_bit"   # n <= x(R) < p: r' = x - n; (r', n - s); (x - n) ^ (1 << b), b in 0..128
WRAP_UNREDUCED = "wrap_unreduced"                    # r' = x itself: at least n
WRAP_ZERO = "wrap_zero"                              # x(R) = n: r' = 0 (and its twin, s = n)
SMALL_VALID, SMALL_BIT = "small_valid", "small_bit"  # x(R) < 2^128 < p - n: both comparisons run
TOP_VALID, TOP_BIT = "top_valid", "top_bit"          # x(R) = n - 2, the largest x of the curve below n
FILLER = "filler"                                    # valid, random u1, u2
ECDSA_VALID_CLASSES = (ORD_VALID, WRAP_VALID, WRAP_TWIN, SMALL_VALID, TOP_VALID, FILLER)
ECDSA_BIT_CLASSES = {ORD_BIT: range(256), WRAP_BIT: range(129), SMALL_BIT: range(129), TOP_BIT: range(1)}
ECDSA_CLASSES = ECDSA_VALID_CLASSES + tuple(ECDSA_BIT_CLASSES) + (ORD_MINUS_N, ORD_MINUS_N_MODP, PLUS_N, WRAP_UNREDUCED, WRAP_ZERO)
X_WRAP_LOW, X_WRAP_HIGH, X_TOP = N, P - 3, N - 2     # on the curve (checked when the corpus is built); nothing between them and p, n
FILLERS_PER_KEY = 20

# ---- BIP-340 classes
BIP_VALID, BIP_BIT, BIP_ODD, BIP_FILLER = "bip_valid", "bip_bit", "bip_odd", "bip_filler"
BIP_VALID_CLASSES = (BIP_VALID, BIP_FILLER)
BIP_CLASSES = (BIP_VALID, BIP_BIT, BIP_ODD, BIP_FILLER)
BIP_FILLERS_PER_KEY = 30

# ---- recovery classes
REC_VALID = "rec_valid"                  # every valid ECDSA item with its id: 04 || Q
REC_BIT1_CLEARED = "rec_bit1_cleared"    # a wrapped r without bit 1 of the id: x = r, another point or none
REC_OTHER_PARITY = "rec_other_parity"    # a wrapped r with the other y: another key
REC_BIT1_SET = "rec_bit1_set"            # an ordinary r with bit 1 of the id: r + n >= p, no key
REC_CLASSES = (REC_VALID, REC_BIT1_CLEARED, REC_OTHER_PARITY, REC_BIT1_SET)


def b32(x):
    return int(x).to_bytes(32, "big")


def _int(b):
    return int.from_bytes(bytes(b), "big")


def _rows(vals):
    return np.frombuffer(b"".join(vals), np.uint8).reshape(len(vals), -1).copy()


def tagged_hash(tag, *vals):
    th = hashlib.sha256(tag.encode()).digest()
    h = hashlib.sha256(th + th)
    for v in vals:
        h.update(v)
    return h.digest()


def lift_x(oracle, x, odd):
    """the point (65 bytes) with this x and that parity of y, or None"""
    root, ok = oracle.fp_sqrt(b32((x * x * x + 7) % P))
    if not ok:
        return None
    y = _int(root)
    if (y & 1) != odd:
        y = P - y
    return b"\x04" + b32(x) + b32(y)


def key_for(oracle, pt, a, b):
    """Q = (R - a G) / b: R = a G + b Q for a point R chosen by its x"""
    diff = oracle.point_add(pt, oracle.point_neg(oracle.scalar_base_mult_vartime(b32(a))))
    return oracle.scalar_mult_vartime(b32(pow(b, -1, N)), diff)


class _Items:
    def __init__(self):
        self.rows = []

    def add(self, cls, q, u1, u2, rp, pt, accept, parent=-1, bit=-1, twin=False):
        """candidate r' on R = u1 G + u2 Q (`pt`): s = r' / u2, e = u1 s; the twin is (r', n - s), which verifies on -R"""
        s = rp % N * pow(u2, -1, N) % N
        e = u1 * s % N
        y_odd = pt[64] & 1
        if twin:
            s, u1, u2, y_odd = N - s, (-u1) % N, (-u2) % N, y_odd ^ 1
        x = _int(pt[1:33])
        self.rows.append(dict(cls=cls, pub=q[1:], dig=b32(e), r=b32(rp), s=b32(s), u1=u1, u2=u2, x=x, accept=accept, parent=parent, bit=bit,
                              rid=(y_odd | (2 if x >= N else 0)) if cls in ECDSA_VALID_CLASSES else -1))
        return len(self.rows) - 1

    def bits(self, cls, q, u1, u2, pt, accept, parent, which):
        for b in which:
            if accept ^ (1 << b):
                self.add(cls, q, u1, u2, accept ^ (1 << b), pt, accept, parent, b)


def build_ecdsa(oracle, seed=1601):
    t0 = time.perf_counter()
    rng = random.Random(seed)
    it = _Items()
    keys = []                                  # 65-byte points, in the order of the key index
    # ---- ordinary R: three keys with known d (key 0 stored with even Y, key 1 with odd Y)
    d = []
    while len(d) < 3:
        v = rng.randrange(1, N)
        q = oracle.scalar_base_mult_vartime(b32(v))
        if len(d) < 2 and (q[64] & 1) != len(d):
            continue
        d.append(v)
        keys.append(q)
    for k, q in enumerate(keys):
        while True:
            u1, u2 = rng.randrange(1, N), rng.randrange(1, N)
            pt = oracle.double_scalar_mult_basepoint_vartime(b32(u1), b32(u2), q)
            x = _int(pt[1:33])
            if pt[0] and P - N <= x < 2 * N - 2**256:     # (all but 2^-126 of the points: both "minus n" candidates are below n)
                break
        v = it.add(ORD_VALID, q, u1, u2, x, pt, x)
        it.bits(ORD_BIT, q, u1, u2, pt, x, v, range(256) if k < 2 else range(0, 256, 16))
        it.add(ORD_MINUS_N, q, u1, u2, (x - N) % 2**256, pt, x, v)
        it.add(ORD_MINUS_N_MODP, q, u1, u2, x + P - N, pt, x, v)
    # ---- R chosen by its x: wrapped (n <= x < p: the two ends of the window and one inside), small (x < 2^128), x = n - 2
    chosen = [(X_WRAP_LOW, 0), (X_WRAP_HIGH, 1)]
    while len(chosen) < 3:
        x = rng.randrange(N, P)
        if lift_x(oracle, x, 0):
            chosen.append((x, x & 1))
    while len(chosen) < 4:
        x = rng.randrange(1 << 127, 1 << 128)
        if lift_x(oracle, x, 1):
            chosen.append((x, 1))
    chosen.append((X_TOP, 0))
    for x, odd in chosen:
        pt = lift_x(oracle, x, odd)
        assert pt is not None, hex(x)
        a, b = rng.randrange(1, N), rng.randrange(1, N)
        q = key_for(oracle, pt, a, b)
        assert q[0] == 4 and oracle.double_scalar_mult_basepoint_vartime(b32(a), b32(b), q) == pt
        keys.append(q)
        if x >= N:
            acc = x - N
            if acc:
                v = it.add(WRAP_VALID, q, a, b, acc, pt, acc)
                it.add(WRAP_TWIN, q, a, b, acc, pt, acc, twin=True)
            else:
                v = it.add(WRAP_ZERO, q, a, b, 0, pt, 0)
                it.add(WRAP_ZERO, q, a, b, 0, pt, 0, twin=True)
            it.bits(WRAP_BIT, q, a, b, pt, acc, v, range(129))
            it.add(WRAP_UNREDUCED, q, a, b, x, pt, acc, v)
        elif x < P - N:
            v = it.add(SMALL_VALID, q, a, b, x, pt, x)
            it.bits(SMALL_BIT, q, a, b, pt, x, v, range(129))
            it.add(PLUS_N, q, a, b, x + N, pt, x, v)
        else:
            v = it.add(TOP_VALID, q, a, b, x, pt, x)
            it.bits(TOP_BIT, q, a, b, pt, x, v, range(1))
    # ---- fillers: valid signatures under every key, known discrete log or not
    for q in keys:
        for _ in range(FILLERS_PER_KEY):
            a, b = rng.randrange(1, N), rng.randrange(1, N)
            pt = oracle.double_scalar_mult_basepoint_vartime(b32(a), b32(b), q)
            x = _int(pt[1:33])
            assert pt[0] and x < N
            it.add(FILLER, q, a, b, x, pt, x)
    # ---- one fixed order that mixes keys and classes
    order = list(range(len(it.rows)))
    rng.shuffle(order)
    where = {old: new for new, old in enumerate(order)}
    rows = [it.rows[i] for i in order]
    key_bytes = [q[1:] for q in keys]
    c = dict(keys=_rows(key_bytes), d=d, cls=[r["cls"] for r in rows],
             pub=_rows([r["pub"] for r in rows]), dig=_rows([r["dig"] for r in rows]), r=_rows([r["r"] for r in rows]), s=_rows([r["s"] for r in rows]),
             kidx=np.array([key_bytes.index(r["pub"]) for r in rows], np.uint32), rid=np.array([r["rid"] for r in rows], np.int16),
             parent=np.array([where.get(r["parent"], -1) for r in rows], np.int32), bit=np.array([r["bit"] for r in rows], np.int16),
             u1=[r["u1"] for r in rows], u2=[r["u2"] for r in rows], x=[r["x"] for r in rows], accept=[r["accept"] for r in rows])
    c["exp"] = oracle.ecdsa_verify_batch(c["pub"], c["dig"], c["r"], c["s"])
    c["seconds"] = time.perf_counter() - t0
    return c


def build_schnorr(oracle, seed=1602):
    t0 = time.perf_counter()
    rng = random.Random(seed)
    d, pts = [], []
    while len(d) < 3:                          # key 0: d G has even y, key 1: odd y (the key set stores it so), key 2 as it comes
        v = rng.randrange(1, N)
        q = oracle.scalar_base_mult_vartime(b32(v))
        if len(d) < 2 and (q[64] & 1) != len(d):
            continue
        d.append(v)
        pts.append(q)
    d_even = [N - v if q[64] & 1 else v for v, q in zip(d, pts)]       # the secret of the even-y point, which BIP-340 verifies under
    rows = []

    def nonce():
        k = rng.randrange(1, N)
        pt = oracle.scalar_base_mult_vartime(b32(k))
        return (N - k, oracle.point_neg(pt)) if pt[64] & 1 else (k, pt)

    def add(cls, key, k, rb, m, parent=-1, bit=-1):
        pk = pts[key][1:33]
        e = _int(tagged_hash("BIP0340/challenge", rb, pk, m)) % N
        rows.append(dict(cls=cls, key=key, pk=pk, msg=m, sig=rb + b32((k + e * d_even[key]) % N), parent=parent, bit=bit, e=e))
        return len(rows) - 1

    for key in (0, 1):
        k, pt = nonce()
        m, x = rng.randbytes(32), _int(pt[1:33])
        v = add(BIP_VALID, key, k, pt[1:33], m)
        for b in range(256):
            add(BIP_BIT, key, k, b32(x ^ (1 << b)), m, v, b)
        add(BIP_ODD, key, N - k, pt[1:33], m, v)                         # -R': the same x, odd y
    for key in range(3):
        for _ in range(BIP_FILLERS_PER_KEY):
            k, pt = nonce()
            add(BIP_FILLER, key, k, pt[1:33], rng.randbytes(32))
    order = list(range(len(rows)))
    rng.shuffle(order)
    where = {old: new for new, old in enumerate(order)}
    rows = [rows[i] for i in order]
    c = dict(keys=_rows([q[1:] for q in pts]), points=pts, cls=[r["cls"] for r in rows], kidx=np.array([r["key"] for r in rows], np.uint32),
             pk32=_rows([r["pk"] for r in rows]), msgs=_rows([r["msg"] for r in rows]), sig=_rows([r["sig"] for r in rows]),
             parent=np.array([where.get(r["parent"], -1) for r in rows], np.int32), bit=np.array([r["bit"] for r in rows], np.int16),
             e=[r["e"] for r in rows])
    c["exp"] = np.array([1 if oracle.schnorr_verify(bytes(pk), bytes(m), bytes(sg)) else 0 for pk, m, sg in zip(c["pk32"], c["msgs"], c["sig"])], np.uint8)
    c["seconds"] = time.perf_counter() - t0
    return c


def build_recovery(oracle, ec):
    """From the ECDSA batch `ec`: (digest, r, s, id) with the oracle's key record (65 zero bytes where it finds none)"""
    rows = []
    for i, cls in enumerate(ec["cls"]):
        v = int(ec["rid"][i])
        if v < 0:
            continue
        rows.append((REC_VALID, i, v))
        if v & 2:
            rows.append((REC_BIT1_CLEARED, i, v & 1))
            rows.append((REC_OTHER_PARITY, i, v ^ 1))
        elif cls in (ORD_VALID, TOP_VALID):
            rows.append((REC_BIT1_SET, i, v | 2))
    src = np.array([i for _, i, _ in rows])
    c = dict(cls=[k for k, _, _ in rows], src=src, dig=ec["dig"][src].copy(), r=ec["r"][src].copy(), s=ec["s"][src].copy(),
             rid=np.array([v for _, _, v in rows], np.uint8))
    rec = [oracle.ecdsa_recover(bytes(c["dig"][j]), bytes(c["r"][j]), bytes(c["s"][j]), int(c["rid"][j])) for j in range(len(rows))]
    c["exp_ok"] = np.array([q is not None for q in rec], np.uint8)
    c["exp_pub"] = _rows([q if q is not None else bytes(65) for q in rec])
    return c


_CACHE = {}


def corpus(oracle):
    """{"ecdsa", "schnorr", "recovery"}: built once per process"""
    if not _CACHE:
        _CACHE["ecdsa"] = build_ecdsa(oracle)
        _CACHE["schnorr"] = build_schnorr(oracle)
        _CACHE["recovery"] = build_recovery(oracle, _CACHE["ecdsa"])
    return _CACHE


def first_differences(got, exp, cls, limit=8):
    """for an assertion message: index, class, got and expected of the first differing items"""
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    return [(int(i), cls[i], int(got[i]), int(exp[i])) for i in bad[:limit]], len(bad)
