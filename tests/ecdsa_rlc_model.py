"""Big-integer model (over pyref) of the whole-batch check of recoverable ECDSA signatures:

    sum a_i R_i  -  (sum a_i u1_i) G  -  sum over distinct keys Q of (sum_{i: Q_i = Q} a_i u2_i) Q  ==  infinity
    u1_i = e_i / s_i,  u2_i = r_i / s_i (mod n),  R_i = RecoverPoint(r_i, v_i)

and the batches the CPU and GPU tests of it are made from.  An item is a tuple (Q, digest, r, s, v) of a point, 32 bytes
and three integers; a batch for the engine is a dict of uint8 arrays pub (n, 64), digest, r, s (n, 32) and v (n,).
"""
import random

import numpy as np

import pyref
from pyref import G, N, P, add, b32, lift_x, mul, neg


def recover_point(r, v):
    """RecoverPoint: bit 1 of v adds n to r (the result must stay below p), bit 0 is the parity of y; None if there is none"""
    if v > 3 or not 1 <= r < N:
        return None
    x = r + (N if v & 2 else 0)
    return lift_x(x, v & 1) if x < P else None


def scalars(digest, r, s):
    e = int.from_bytes(digest[:32], "big") % N
    w = pow(s, -1, N)
    return e * w % N, r * w % N


def item_error(Q, digest, r, s, v):
    """E_i = R_i - u1_i G - u2_i Q_i: the identity (None) exactly for a good item with a key on the curve"""
    u1, u2 = scalars(digest, r, s)
    return add(recover_point(r, v), neg(add(mul(u1, G), mul(u2, Q))))


def is_good(Q, digest, r, s, v, reject_malleable=False):
    if not (1 <= r < N and 1 <= s < N) or v > 3 or (reject_malleable and s > N // 2):
        return False
    if Q is None or not (Q[0] < P and Q[1] < P and pyref.on_curve(Q)) or recover_point(r, v) is None:
        return False
    return item_error(Q, digest, r, s, v) is None


def combination(items, coeffs):
    """the sum as the engine forms it: one term per R_i, one for G, one per DISTINCT key"""
    acc, g_coeff, per_key = None, 0, {}
    for (Q, digest, r, s, v), a in zip(items, coeffs):
        u1, u2 = scalars(digest, r, s)
        acc = add(acc, mul(a, recover_point(r, v)))
        g_coeff = (g_coeff + a * u1) % N
        per_key[Q] = (per_key.get(Q, 0) + a * u2) % N
    acc = add(acc, neg(mul(g_coeff, G)))
    for Q, c in per_key.items():
        acc = add(acc, neg(mul(c, Q)))
    return acc


def in_combination(Q, digest, r, s, v, reject_malleable=False):
    """the item passes its own checks: ranges of r, s and v, low s under the flag, a point for (r, v), a key on the curve"""
    if not (1 <= r < N and 1 <= s < N) or v > 3 or (reject_malleable and s > N // 2):
        return False
    return Q is not None and Q[0] < P and Q[1] < P and pyref.on_curve(Q) and recover_point(r, v) is not None


def item_error_with(ar, Q, digest, r, s, v):
    """item_error over another implementation of the group (schnorr_rlc_model.Arith)"""
    u1, u2 = scalars(digest, r, s)
    return ar.add(recover_point(r, v), neg(ar.add(ar.base_mult(u1), ar.mul(u2, Q))))


OUT = "out of the combination"


def checked_error(item, ar=None, reject_malleable=False, errors=None):
    """E_i of an item that is in the combination, OUT for one that is not; kept in `errors` (a dict) by item and flag"""
    import schnorr_rlc_model as SM
    key = (item, reject_malleable)
    if errors is None or key not in errors:
        E = item_error_with(ar or SM.PURE, *item) if in_combination(*item, reject_malleable=reject_malleable) else OUT
        if errors is None:
            return E
        errors[key] = E
    return errors[key]


def error_point(items, key32, lo=0, cnt=None, ar=None, reject_malleable=False, errors=None):
    """(E, status): E = sum a_i R_i - (sum a_i u1_i) G - sum (a_i u2_i) Q_i = sum of a_i E_i over the items lo <= i < lo + cnt
    that are in the combination, a_i = schnorr_rlc_model.coefficient(key32, i) by the index in the batch; status = some item
    of the range is out of the combination.  errors: a dict that keeps E_i by item across calls (tiled batches)."""
    import schnorr_rlc_model as SM
    ar = ar or SM.PURE
    cnt = len(items) - lo if cnt is None else cnt
    acc, status = None, False
    for i in range(lo, lo + cnt):
        E = checked_error(items[i], ar, reject_malleable, errors)
        if E is OUT:
            status = True
        elif E is not None:
            acc = ar.add(acc, ar.mul(SM.coefficient(key32, i), E))
    return acc, status


def from_arrays(b):
    """the items of an engine batch (a key that is no point stays a pair of integers)"""
    val = lambda row: int.from_bytes(bytes(row), "big")
    return [((val(b["pub"][i][:32]), val(b["pub"][i][32:])), bytes(b["digest"][i]), val(b["r"][i]), val(b["s"][i]), int(b["v"][i]))
            for i in range(len(b["v"]))]


def sign_recoverable(d, digest, k, high_s=False, base_mult=None):
    """(r, s, v) of the nonce k: v = parity of y(k G), flipped when s is negated, bit 1 set when x(k G) >= n"""
    R = base_mult(k) if base_mult else mul(k, G)
    e = int.from_bytes(digest[:32], "big") % N
    r = R[0] % N
    s = pow(k, -1, N) * (e + r * d) % N
    v = (R[1] & 1) | (2 if R[0] >= N else 0)
    if (s > N // 2) != high_s:
        s, v = N - s, v ^ 1
    return r, s, v


def make_recoverable_items(n, nkeys, seed, high_s_every=0, base_mult=None):
    """n good items under nkeys keys (item i under key i mod nkeys); every high_s_every-th has s > n/2"""
    rng = random.Random(seed)
    bm = base_mult or (lambda k: mul(k, G))
    ds = [rng.randrange(1, N) for _ in range(nkeys)]
    Qs = [bm(d) for d in ds]
    items = []
    for i in range(n):
        digest = rng.randbytes(32)
        high = bool(high_s_every) and i % high_s_every == high_s_every - 1
        r, s, v = sign_recoverable(ds[i % nkeys], digest, rng.randrange(1, N), high, base_mult)
        items.append((Qs[i % nkeys], digest, r, s, v))
    return items


def to_arrays(items):
    u8 = lambda rows, w: np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(-1, w).copy()
    return {"pub": u8([b32(Q[0]) + b32(Q[1]) for Q, _, _, _, _ in items], 64),
            "digest": u8([dg for _, dg, _, _, _ in items], 32),
            "r": u8([b32(r) for _, _, r, _, _ in items], 32),
            "s": u8([b32(s) for _, _, _, s, _ in items], 32),
            "v": np.array([v for _, _, _, _, v in items], dtype=np.uint8)}


def make_recoverable_batch(n, nkeys, seed, high_s_every=0, base_mult=None):
    return to_arrays(make_recoverable_items(n, nkeys, seed, high_s_every, base_mult))


def cancelling_pair(seed, base_mult=None):
    """one good (digest, r, s, v) of the key Q, offered under Q + D and under Q - D: the two errors are -u2 D and +u2 D"""
    (Q, digest, r, s, v), = make_recoverable_items(1, 1, seed, base_mult=base_mult)
    D = mul(random.Random(seed + 1).randrange(1, N), G)
    return (add(Q, D), digest, r, s, v), (add(Q, neg(D)), digest, r, s, v)


def high_x_tuple(seed):
    """(digest, r, s): r = x - n for the first x > n that is the abscissa of a point of the curve (x = n itself would make
    r = 0); with bit 1 of v set the signature's R is that point.  The key comes from the recovery, whatever s and digest are."""
    x = N + 1
    while lift_x(x, 0) is None:
        x += 1
    rng = random.Random(seed)
    return rng.randbytes(32), x - N, rng.randrange(1, N // 2)


def recover_key(digest, r, s, v):
    """RecoverPublicKey in big integers: Q = (s R - e G) / r, None where the reference fails"""
    R = recover_point(r, v)
    if R is None or not 1 <= s < N:
        return None
    e = int.from_bytes(digest[:32], "big") % N
    return mul(pow(r, -1, N), add(mul(s, R), neg(mul(e, G))))
