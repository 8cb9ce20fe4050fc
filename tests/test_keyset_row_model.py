"""The addition the wave-per-signature key-set ladder runs (csrc/fe29r.h: pt29r_add_b3, pt29r_from_iso; small_call.hip:
row_ladder_keyset) on the lane-level model tests/fer_b3_model.py: values against big-integer arithmetic on the key's
isomorphic curve y^2 = x^3 + 7 W^6, limb bounds at the top of what the ladder feeds it, and the whole ladder - lead pair, 64
digit additions, the map back, the generator part - against u1 G + u2 Q for the recoding's corner scalars.  No GPU; the
compiled functions run in tests/test_gpu_keyset_row.py."""
import random

import fer_b3_model as B
import fer_model as F
import pyref as R
from test_fer_model import BOUND1, affine, lazy, proj

P = F.P


def to_iso(pt, w):
    return None if pt is None else (pt[0] * w * w % P, pt[1] * pow(w, 3, P) % P)


def on_iso(pt, w):
    return pt is None or (pt[1] ** 2 - pt[0] ** 3 - 7 * pow(w, 6, P)) % P == 0


def test_ptr_add_b3_is_the_group_law_of_the_isomorphic_curve():
    """P + Q, P + P, P + (-P), the identity on either side and on both, for random W, projective scalings and y with one and
    two units: the complete formula has no exceptional case, and its b3 is 21 W^6."""
    rnd = random.Random(1401)
    for it in range(48):
        w = rnd.randrange(1, P)
        p = R.mul(rnd.randrange(1, R.N), R.G)
        q = R.mul(rnd.randrange(1, R.N), R.G)
        case = it % 8
        if case == 1:
            q = p
        elif case == 2:
            q = R.neg(p)
        elif case == 3:
            p = None
        elif case == 4:
            q = None
        elif case == 5:
            p = q = None
        pi, qi = to_iso(p, w), to_iso(q, w)
        assert on_iso(pi, w) and on_iso(qi, w)
        _, _, b3 = B.iso_consts(lazy(w, rnd))
        assert F.fer_value(b3) % P == 21 * pow(w, 6, P) % P and all(b3[j] <= BOUND1[j] for j in range(9))
        P1 = proj(pi, rnd.randrange(1, P), rnd, 1 + it % 2)
        Q1 = proj(qi, 1 if it % 3 == 0 else rnd.randrange(1, P), rnd, 1 + (it // 2) % 2)     # (table entries come with Z = 1)
        got = B.ptr_add_b3(P1, Q1, b3)
        assert affine(*got) == R.add(pi, qi), (it, case)        # (the affine law contains no curve constant: pyref's serves)
        for c in got:
            for row in range(4):
                assert all(c[16 * row + j] <= BOUND1[j] for j in range(9))
        # a chain on its own output, then back to secp256k1
        acc, ref = got, R.add(pi, qi)
        for _ in range(3):
            acc = B.ptr_add_b3(acc, Q1, b3)
            ref = R.add(ref, qi)
        wv, w3, _ = B.iso_consts(lazy(w, rnd))
        back = affine(*B.ptr_from_iso(acc, wv, w3))
        exp = R.add(R.add(p, q), R.mul(3, q)) if q is not None else p
        assert back == exp and to_iso(back, w) == ref
    # the plain curve is the case W = 1
    p, q = R.mul(5, R.G), R.mul(7, R.G)
    _, _, b3 = B.iso_consts(lazy(1, rnd))
    assert F.fer_value(b3) == 21
    assert affine(*B.ptr_add_b3(proj(p, 3, rnd), proj(q, 1, rnd), b3)) == R.mul(12, R.G) == affine(*F.ptr_add(proj(p, 3, rnd), proj(q, 1, rnd)))


def test_ptr_add_b3_limb_bounds():
    """Every intermediate of the new layers stays within what fer_mul_tail accepts: the model asserts each 32- / 64-bit width
    inside its products (fer_model._tail, fer_carry), so running the formula with every input limb at the TOP of its budget -
    X, Z and b3 one unit, Y two units, what the ladder's negated table entries and a doubling's output bring - is the proof;
    the outputs are one unit again, so the bound holds along a chain."""
    top = lambda u: F.lane_const(lambda j, r: u * BOUND1[j] if j <= 8 else 0)
    Pt = (top(1), top(2), top(1))
    out = B.ptr_add_b3(Pt, Pt, top(1))
    for c in out:
        assert all(c[l] <= BOUND1[l & 15] for l in range(F.LANES) if (l & 15) <= 8)
        assert all(c[l] == 0 for l in range(F.LANES) if (l & 15) > 8)
    out2 = B.ptr_add_b3(out, Pt, top(1))           # ... and fed back
    for c in out2:
        assert all(c[l] <= BOUND1[l & 15] for l in range(F.LANES) if (l & 15) <= 8)
    w, w3, b3 = B.iso_consts(top(1))
    for c in (w3, b3) + B.ptr_from_iso(out, w, w3):
        assert all(c[l] <= BOUND1[l & 15] for l in range(F.LANES) if (l & 15) <= 8)
    # the budget of the last layer is the formula's own: [2] x [3] + [1] x [1] = 7 units
    assert 2 * 3 + 1 * 1 <= 7


def key_table(q, w):
    """the 32-chunk table of key q on the curve isomorphic by w (engine_internal.h: kt_geom<32>): entry 8 c + j =
    (2 j + 1) 16^c Q, and the lead pair L + phi(L), L - phi(L), L = 16^32 Q; each with its endomorphism image's x"""
    phi = lambda pt: (pt[0] * R.BETA % P, pt[1])
    tab = []
    for c in range(32):
        base = R.mul(16 ** c, q)
        for j in range(8):
            tab.append(to_iso(R.mul(2 * j + 1, base), w))
    L = R.mul(16 ** 32, q)
    tab.append(to_iso(R.add(L, phi(L)), w))
    tab.append(to_iso(R.add(L, R.neg(phi(L))), w))
    return tab


def model_ladder(tab, w, k1, neg1, k2, neg2, u1, rnd):
    """row_ladder_keyset on the model: the digits of k_verify_fast<MODE_ECDSA_KEYSET> (nibble c of (k - 1) / 2 is the signed odd
    digit 2 nib - 15 of chunk c), the lead pair first, 64 additions on the isomorphic curve, the map back, + u1 G"""
    wv, w3, b3 = B.iso_consts(lazy(w, rnd))
    beta_w = lambda pt: (pt[0] * R.BETA % P, pt[1])      # (beta x of the isomorphic point is the image's x there too)
    lead = tab[256 if neg1 == neg2 else 257]
    if neg1:
        lead = R.neg(lead)
    acc = proj(lead, 1, rnd)
    a, b = (k1 - 1) // 2, (k2 - 1) // 2
    for c in range(32):
        for half, (val, sneg) in enumerate(((a, neg1), (b, neg2))):
            nib = (val >> (4 * c)) & 15
            e = tab[8 * c + (7 - nib if nib < 8 else nib - 8)]
            if half:
                e = beta_w(e)
            if sneg != (nib < 8):
                e = R.neg(e)
            acc = B.ptr_add_b3(acc, proj(e, 1, rnd, 2), b3)      # (a negated entry's y has two units)
    acc = B.ptr_from_iso(acc, wv, w3)
    g = R.mul(u1, R.G)
    return affine(*F.ptr_add(acc, proj(g, 1, rnd))) if g is not None else affine(*acc)


def test_ladder_corner_scalars():
    """The map back (X' W : Y' : Z' W^3) followed by the generator addition is u1 G + u2 Q for the corner half scalars of the
    recoding: 1 (all digits -15), 2^128 + 1 (top digit +1), 2^129 - 1 (all digits +15), with every sign pair met once."""
    rnd = random.Random(1402)
    q = R.mul(rnd.randrange(1, R.N), R.G)
    w = rnd.randrange(2, P)
    tab = key_table(q, w)
    cases = [(1, False, 1, False), (2 ** 128 + 1, True, 1, False), (2 ** 129 - 1, False, 2 ** 129 - 1, True), (1, True, 2 ** 128 + 1, True)]
    for k1, n1, k2, n2 in cases:
        u2 = ((-k1 if n1 else k1) + (-k2 if n2 else k2) * R.LAMBDA) % R.N
        u1 = rnd.randrange(R.N) if k1 != 1 or n1 else 0
        exp = R.add(R.mul(u1, R.G), R.mul(u2, q))
        assert model_ladder(tab, w, k1, n1, k2, n2, u1, rnd) == exp, (hex(k1), n1, hex(k2), n2)
    # R = identity: the key part is minus the generator part, and the complete addition says so (Z = 0)
    k1, n1, k2, n2 = 2 ** 129 - 1, False, 1, False
    u2 = (k1 + k2 * R.LAMBDA) % R.N
    d = rnd.randrange(1, R.N)
    tab = key_table(R.mul(d, R.G), w)
    assert model_ladder(tab, w, k1, n1, k2, n2, (-u2 * d) % R.N, rnd) is None
