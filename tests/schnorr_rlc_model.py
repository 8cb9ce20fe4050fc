"""Big-integer model of the whole-batch check of BIP-340 signatures and of the value its bisection computes with:

    E = sum over the items in the combination of a_i E_i,    E_i = s_i G - lift_x(r_i) - e_i lift_x(pk_i)
    a_0 = 1,  a_i = the low 128 bits of SHA-256(key || i as 8 bytes, big-endian),  e_i = the tagged challenge hash mod n

restated from BIP-340's verification equation (s G = R + e P, R and P the even-y points of r and pk), and the batches the
CPU and GPU tests of it are made from.  An item is a tuple (pk, msg, sig) of 32 bytes, any bytes and 64 bytes; a batch for the
engine is a dict pk (n, 32) and sig (n, 64) uint8 arrays and msgs, a list of byte strings.  Points are pyref's: (x, y) or
None for the identity.  The group arithmetic is pyref's (PURE) or, behind the same three functions and much faster, the C
oracle's (oracle_arith): the equation is the same, only who adds the points differs.
"""
import hashlib
import random

import numpy as np

import pyref
from pyref import G, N, P, b32, lift_x, neg

OUT = "out of the combination"          # what item_error returns for an item the preparation leaves out


class Arith:
    """base_mult(k) = k G, mul(k, pt), add(a, b) on pyref's points"""

    def __init__(self, base_mult, mul, add):
        self.base_mult, self.mul, self.add = base_mult, mul, add


PURE = Arith(lambda k: pyref.mul(k, G), pyref.mul, pyref.add)


def oracle_arith(oracle):
    enc, dec = pyref.enc65, pyref.dec65
    return Arith(lambda k: dec(oracle.scalar_base_mult_vartime(b32(k % N))),
                 lambda k, pt: dec(oracle.scalar_mult_vartime(b32(k % N), enc(pt))),
                 lambda a, b: dec(oracle.point_add(enc(a), enc(b))))


def coefficient(key32, i):
    if i == 0:
        return 1
    return int.from_bytes(hashlib.sha256(key32 + i.to_bytes(8, "big")).digest()[16:], "big")


def parts(item):
    pk, msg, sig = item
    return int.from_bytes(pk, "big"), int.from_bytes(sig[:32], "big"), int.from_bytes(sig[32:], "big")


def in_combination(pk, msg, sig):
    """r < p and r lifts, s < n (s = 0 is allowed, as in BIP-340), pk < p and pk lifts"""
    x, r, s = parts((pk, msg, sig))
    return lift_x(r, 0) is not None and s < N and lift_x(x, 0) is not None          # (lift_x refuses x >= p)


def challenge(pk, msg, sig):
    return int.from_bytes(pyref.tagged_hash("BIP0340/challenge", sig[:32], pk, msg), "big") % N


def item_error(pk, msg, sig, ar=PURE):
    """E_i = s G - lift_x(r) - e lift_x(pk): the identity (None) exactly for an item BIP-340 accepts; OUT for an item that is
    not in the combination (it is rejected too)"""
    if not in_combination(pk, msg, sig):
        return OUT
    x, r, s = parts((pk, msg, sig))
    e = challenge(pk, msg, sig)
    acc = ar.add(ar.base_mult(s), neg(lift_x(r, 0)))
    return ar.add(acc, neg(ar.mul(e, lift_x(x, 0))))


class Errors:
    """item_error by the item's bytes, computed once: tiled batches repeat their items"""

    def __init__(self, ar=PURE):
        self.ar, self.seen = ar, {}

    def __call__(self, item):
        key = (bytes(item[0]), bytes(item[1]), bytes(item[2]))
        if key not in self.seen:
            self.seen[key] = item_error(*key, ar=self.ar)
        return self.seen[key]


def error_point(items, key32, lo=0, cnt=None, ar=PURE, errors=None):
    """(E, status): E = sum of a_i E_i over the items lo <= i < lo + cnt that are in the combination, a_i by the index in
    the batch; status = some item of the RANGE is out of the combination (the device's status word is the preparation's and
    covers the whole batch: compare it with the status of the range (0, n), whatever range the point is of)"""
    errors = errors or Errors(ar)
    cnt = len(items) - lo if cnt is None else cnt
    acc, status = None, False
    for i in range(lo, lo + cnt):
        E = errors(items[i])
        if E is OUT:
            status = True
        elif E is not None:
            acc = ar.add(acc, ar.mul(coefficient(key32, i), E))
    return acc, status


def in_combination_flags(items):
    return np.array([1 if in_combination(*it) else 0 for it in items], np.uint8)


# ---- batches ----
def even_secret(d, ar=PURE):
    """(the secret of the even-y point with d G's abscissa, that abscissa as 32 bytes)"""
    Q = ar.base_mult(d)
    return (N - d if Q[1] & 1 else d), b32(Q[0])


def sign(d_even, pk, msg, k, ar=PURE):
    """the signature with the nonce +-k (the one of the two whose point has an even y)"""
    R = ar.base_mult(k)
    if R[1] & 1:
        k = N - k
    e = challenge(pk, msg, b32(R[0]))
    return b32(R[0]) + b32((k + e * d_even) % N)


def make_keys(nkeys, rng, ar=PURE):
    """nkeys (even secret, x-only key, secret as drawn); key 0 comes from a point with an even y, key 1 from one with an odd y"""
    keys = []
    while len(keys) < nkeys:
        d = rng.randrange(1, N)
        if len(keys) < 2 and (ar.base_mult(d)[1] & 1) != len(keys):
            continue
        keys.append(even_secret(d, ar) + (d,))
    return keys


def make_items(n, nkeys, seed, msg_lens=(32,), ar=PURE):
    """n good items: item i under key i mod nkeys, its message msg_lens[i mod len(msg_lens)] bytes long"""
    rng = random.Random(seed)
    keys = make_keys(nkeys, rng, ar)
    items = []
    for i in range(n):
        d_even, pk, _ = keys[i % nkeys]
        msg = rng.randbytes(msg_lens[i % len(msg_lens)])
        items.append((pk, msg, sign(d_even, pk, msg, rng.randrange(1, N), ar)))
    return items


def to_arrays(items):
    u8 = lambda rows, w: np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, w).copy()
    return {"pk": u8([bytes(it[0]) for it in items], 32), "sig": u8([bytes(it[2]) for it in items], 64),
            "msgs": [bytes(it[1]) for it in items]}


def with_s(item, s):
    pk, msg, sig = item
    return pk, msg, sig[:32] + b32(s)


def cancelling_pair(item_i, item_j, delta):
    """two good items offered as (r_i, s_i + delta) and (r_j, s_j - delta): their errors are delta G and -delta G"""
    si, sj = parts(item_i)[2], parts(item_j)[2]
    return with_s(item_i, (si + delta) % N), with_s(item_j, (sj - delta) % N)


def exceptional_items(seed, ar=PURE):
    """Good items whose terms meet in the sum, under one key d (and G itself as the second key, for P = G):
    [0, 64) the same signature 64 times; 64, 65: one nonce, two messages; 66: R = G (k = 1); 67: P = G (d = 1) - so item 66's R
    is item 67's key point; 68: R = P (k = the even-y secret); 69: R = G under the key G (R = P = G)."""
    rng = random.Random(seed)
    d_even, pk, _ = make_keys(1, rng, ar)[0]
    msg = [rng.randbytes(32) for _ in range(8)]
    k = rng.randrange(1, N)
    one = b32(G[0])
    return ([(pk, msg[0], sign(d_even, pk, msg[0], rng.randrange(1, N), ar))] * 64
            + [(pk, msg[1], sign(d_even, pk, msg[1], k, ar)), (pk, msg[2], sign(d_even, pk, msg[2], k, ar)),
               (pk, msg[3], sign(d_even, pk, msg[3], 1, ar)),
               (one, msg[4], sign(1, one, msg[4], rng.randrange(1, N), ar)),
               (pk, msg[5], sign(d_even, pk, msg[5], d_even, ar)),
               (one, msg[6], sign(1, one, msg[6], 1, ar))])


def first_non_abscissa(start=2):
    x = start
    while lift_x(x, 0) is not None:
        x += 1
    return x


def flip_bit_of_r(item, want_lift):
    """the item with the lowest bit of r flipped after which r still lifts (want_lift) or no longer does"""
    pk, msg, sig = item
    r = int.from_bytes(sig[:32], "big")
    for b in range(256):
        x = r ^ (1 << b)
        if (lift_x(x, 0) is not None) == want_lift:
            return pk, msg, b32(x) + sig[32:]
    raise AssertionError("no such bit")


def damages(items, i):
    """{name: the batch with item i damaged that way}: every way to be bad of tests/test_gpu_schnorr_rlc.py, test 4"""
    pk, msg, sig = items[i]
    r, s = sig[:32], int.from_bytes(sig[32:], "big")
    other = next(it[0] for it in items[i + 1:] + items[:i] if it[0] != pk)
    out = {
        "s = n": (pk, msg, r + b32(N)),
        "s = n + 1": (pk, msg, r + b32(N + 1)),
        "s = 2^256 - 1": (pk, msg, r + b32(2**256 - 1)),
        "a bit of s": (pk, msg, r + b32(s ^ (1 << 77))),
        "r = p": (pk, msg, b32(P) + sig[32:]),
        "r = p + 1": (pk, msg, b32(P + 1) + sig[32:]),
        "r = a non-abscissa": (pk, msg, b32(first_non_abscissa()) + sig[32:]),
        "a bit of r that lifts": flip_bit_of_r(items[i], True),
        "a bit of r that does not lift": flip_bit_of_r(items[i], False),
        "pk = p": (b32(P), msg, sig),
        "pk = a non-abscissa": (b32(first_non_abscissa()), msg, sig),
        "pk = another valid key": (other, msg, sig),
        "a bit of the message": (pk, bytes([msg[0] ^ 0x20]) + msg[1:], sig),
        "the message one byte shorter": (pk, msg[:-1], sig),
    }
    res = {}
    for name, item in out.items():
        bad = list(items)
        bad[i] = item
        res[name] = bad
    return res
