"""Model of the comb tables of the ECDSA flow and of the ladder over them (engine_internal.h: kc_geom; keyed.hip:
coz29_conj, kc_sets, k_key_finish_comb; verify_fast.h: k_verify_fast<MODE_ECDSA_COMB>), without a GPU:

  * the recoding: an odd half scalar k < 2^129 as 2^133 + sum b_i 2^i, b_i = 2 a_i - 1, a = k >> 1, read column by column
    through seven teeth 19 bits apart - the digits exactly as the kernel forms them, their sum, the operation counts;
  * coz29_conj (P + Q and P - Q of two points over one Z): interval bounds in the units of fe29.h, the schedule limb by
    limb at the bounds' edge, its values against affine arithmetic, and a drift guard against the C++ body;
  * the build: k_key_chain on the comb's geometry with kc_sets, and k_key_finish_comb, on VALUES for whole keys - bases
    onto one Z by prefix / suffix products, the A and C sets, the 64 entries and the lead pair, the index of every entry and the shared W - against
    tests/pyref.py; their interval bounds over the kernels' own call sequences (drift-guarded).
"""
import random
import re

import pytest

import pyref as R
import test_fe29_formulas_model as fm
import test_fe29_model as m
from test_fe29_formulas_model import COORD, NW, PROD, Y2, from_words, group_shl, le, select, within, zero
from test_coz_model import group_shr
from test_fe29_model import P, add, cpp, mul, mul_plus, negate, normalize_weak, sqr, sqr_plus

N = R.N
TEETH, SPACING, LEN, LEAD_LOG2 = 7, 19, 133, 115


def _const(name, fname="engine_internal.h"):
    mt = re.search(r"\b%s\s*=\s*(0x[0-9a-fA-F]+|\d+)" % name, fm.source(fname))
    assert mt, name
    return int(mt.group(1), 0)


def test_geometry_is_the_source_s():
    src = fm.source("engine_internal.h")
    assert re.search(r"TEETH = 7, SPACING = 19, LEN = TEETH \* SPACING", src)
    assert re.search(r"LEAD_LOG2 = LEN - SPACING \+ 1", src) and re.search(r"LEAD = 64, ENTRIES = 66", src)
    assert LEN == TEETH * SPACING and LEAD_LOG2 == LEN - SPACING + 1 == (TEETH - 1) * SPACING + 1


# ==== the recoding ======================================================================================================
def comb_digits(k):
    """[(entry, negative)] of the 19 rounds j = 18 .. 0 for the odd half scalar k, formed as k_verify_fast<MODE_ECDSA_COMB>
    forms them: teeth from the words of k, bit j of each, the top tooth's bit as the sign"""
    assert k & 1 and 0 < k < 1 << 129
    words = [(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    teeth = []
    for t in range(TEETH):
        bit = SPACING * t + 1
        limb, sh = bit >> 5, bit & 31
        v = words[limb] >> sh
        if sh > 32 - SPACING:
            v |= (words[limb + 1] << (32 - sh)) & 0xFFFFFFFF
        teeth.append(v & ((1 << SPACING) - 1))
    out = []
    for j in range(SPACING - 1, -1, -1):
        w = 0
        for t in range(TEETH):
            w |= ((teeth[t] >> j) & 1) << t
        top = bool(w & 64)
        out.append(((w if top else ~w) & 63, not top))
    return out


def entry_scalar(idx):
    """E[idx] = B_6 + sum_{t<6} (2 idx_t - 1) B_t as a multiple of Q, B_t = 2^(19 t) Q"""
    return (1 << (SPACING * 6)) + sum((2 * ((idx >> t) & 1) - 1) << (SPACING * t) for t in range(6))


def ladder_scalar(k):
    """what the ladder computes, as a multiple of Q; (additions, doublings)"""
    acc, adds, dbls = 1 << LEAD_LOG2, 0, 0
    for r, (entry, negative) in enumerate(comb_digits(k)):
        if r:
            acc *= 2
            dbls += 1
        assert 0 <= entry < 64
        acc += -entry_scalar(entry) if negative else entry_scalar(entry)
        adds += 1
    return acc, adds, dbls


BOUNDARY_HALVES = [1, 3, 2**128 - 1, 2**128 + 1, 2**129 - 1]


def half_scalars():
    ks = list(BOUNDARY_HALVES)
    ks += [2 * a + 1 for a in (0, 2**128 - 1)] + [2 * (1 << b) + 1 for b in range(128)]            # a = 0, all ones, single bits
    ks += [2 * ((1 << 128) - 1 - (1 << b)) + 1 for b in range(128)]                                  # a single zero bit
    ks += [2 * sum(1 << (SPACING * t + j) for t in range(TEETH) if SPACING * t + j < 128) + 1 for j in range(SPACING)]   # a full column
    rng = random.Random(1907)
    ks += [rng.randrange(1 << 129) | 1 for _ in range(3000)]
    ks += [rng.randrange(1 << rng.randrange(1, 130)) | 1 for _ in range(1000)]
    return ks


def test_recoding_sums_to_the_scalar():
    for k in half_scalars():
        got, adds, dbls = ladder_scalar(k)
        assert got == k, hex(k)
        assert (adds, dbls) == (SPACING, SPACING - 1) == (19, 18)
    # the lead: 2^115 Q, doubled 18 times, is the recoding's 2^133
    assert (1 << LEAD_LOG2) << (SPACING - 1) == 1 << LEN


def test_recoding_is_the_signed_bit_form():
    """the same digits from the definition: b_i = 2 a_i - 1 over i = 19 t + j, the column's sum as +- an entry"""
    rng = random.Random(5)
    for k in BOUNDARY_HALVES + [rng.randrange(1 << 129) | 1 for _ in range(300)]:
        a = k >> 1
        for r, (entry, negative) in enumerate(comb_digits(k)):
            j = SPACING - 1 - r
            col = sum((2 * ((a >> (SPACING * t + j)) & 1) - 1) << (SPACING * t) for t in range(TEETH))
            assert col == (-1 if negative else 1) * entry_scalar(entry)


def test_every_entry_and_sign_is_reachable():
    rng = random.Random(6)
    seen = set()
    for _ in range(400):
        seen |= set(comb_digits(rng.randrange(1 << 129) | 1))
    assert len(seen) == 128


# ==== coz29_conj: bounds ================================================================================================
@cpp("coz29_conj")
def coz_conj(p, q):
    (px, py), (qx, qy) = p, q
    h = normalize_weak(add(qx, negate(px, 1)))
    a = sqr(h)
    b = mul(px, a)
    c = mul(qx, a)
    nbc = negate(add(b, c), 2)
    ne = negate(mul(py, add(c, negate(b, 1))), 1)
    dy = normalize_weak(add(qy, negate(py, 1)))
    sx = sqr_plus(dy, nbc)
    sy = mul_plus(dy, add(b, negate(sx, 1)), ne)
    ny = normalize_weak(negate(add(qy, py), 2))
    dx = sqr_plus(ny, nbc)
    dyy = mul_plus(ny, add(b, negate(dx, 1)), ne)
    return (sx, sy), (dx, dyy), h


@cpp("coz29_rescale")
def coz_rescale(p, c2, c3):
    return (mul(p[0], c2), mul(p[1], c3))


APT = (COORD, COORD)                       # an apt29: x [1], y [1]


def test_conj_invariant_closed():
    s, d, h = coz_conj(APT, APT)
    assert within(s, APT) and within(d, APT) and le(h, COORD)
    s2, d2, h2 = coz_conj(s, d)             # results feed the next level
    assert within(s2, APT) and within(d2, APT) and le(h2, COORD)
    assert within(coz_rescale((COORD, Y2), COORD, COORD), APT)       # a jpt29's y [<= 2] is taken
    with pytest.raises(AssertionError):
        coz_conj((COORD, m.B.units(2.5)), APT)                       # negate(p.y, 1) needs y [1]
    with pytest.raises(AssertionError):
        coz_conj(APT, (COORD, m.B.units(2.5)))                       # negate(q.y + p.y, 2)


# ==== coz29_conj: the schedule limb by limb, and its values ==============================================================
def _add(a, b):
    r = [x + y for x, y in zip(a, b)]
    assert all(x < m.U32 for x in r)
    return r


def conj_int(p, q):
    (px, py), (qx, qy) = p, q
    h = m.normalize_weak_int(_add(qx, m.negate_int(px, 1)))
    a = m.mulsum_int([(h, h)])
    b = m.mulsum_int([(px, a)])
    c = m.mulsum_int([(qx, a)])
    nbc = m.negate_int(_add(b, c), 2)
    ne = m.negate_int(m.mulsum_int([(py, _add(c, m.negate_int(b, 1)))]), 1)
    dy = m.normalize_weak_int(_add(qy, m.negate_int(py, 1)))
    sx = m.mulsum_int([(dy, dy)], nbc)
    sy = m.mulsum_int([(dy, _add(b, m.negate_int(sx, 1)))], ne)
    ny = m.normalize_weak_int(m.negate_int(_add(qy, py), 2))
    dx = m.mulsum_int([(ny, ny)], nbc)
    dyy = m.mulsum_int([(ny, _add(b, m.negate_int(dx, 1)))], ne)
    return (sx, sy), (dx, dyy), h


def _affine(X, Y, Z):
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi * zi * zi % P


def test_conj_gives_sum_and_difference():
    rng = random.Random(2711)
    for it in range(40):
        a, b = R.mul(rng.randrange(1, N), R.G), R.mul(rng.randrange(1, N), R.G)
        z = rng.randrange(1, P)                                    # both over one Z
        p = (m.from_int(a[0] * z * z % P), m.from_int(a[1] * z ** 3 % P))
        q = (m.from_int(b[0] * z * z % P), m.from_int(b[1] * z ** 3 % P))
        s, d, h = conj_int(p, q)
        z3 = z * m.value(h) % P
        assert _affine(m.value(s[0]), m.value(s[1]), z3) == R.add(a, b), it
        assert _affine(m.value(d[0]), m.value(d[1]), z3) == R.add(a, R.neg(b)), it
        assert all(x <= m.M + (1 << 20) for v in s + d for x in v)


def test_conj_on_extremal_limbs():
    """every limb of every operand at the invariant's bound: the formulas as polynomials"""
    rng = random.Random(13)
    for it in range(200):
        p = (m.rand_lazy(rng, 1, it % 2 == 0), m.rand_lazy(rng, 1, it % 2 == 0))
        q = (m.rand_lazy(rng, 1, it % 3 == 0), m.rand_lazy(rng, 1, it % 3 == 0))
        px, py, qx, qy = (m.value(v) for v in p + q)
        s, d, h = conj_int(p, q)
        hv = (qx - px) % P
        Bv, C = px * hv * hv % P, qx * hv * hv % P
        for (x3, y3), y2 in ((s, qy), (d, -qy)):
            X = ((y2 - py) ** 2 - Bv - C) % P
            assert m.value(x3) % P == X and m.value(y3) % P == ((y2 - py) * (Bv - X) - py * (C - Bv)) % P
        assert m.value(h) % P == hv


# ==== the build on values ================================================================================================
def _conj(p, q):
    (px, py), (qx, qy) = p, q
    h = (qx - px) % P
    a = h * h % P
    b, c = px * a % P, qx * a % P
    e = py * (c - b) % P
    out = []
    for y2 in (qy, -qy):
        x3 = ((y2 - py) ** 2 - b - c) % P
        out.append((x3, ((y2 - py) * (b - x3) - e) % P))
    return out[0], out[1], h


def _rescale(p, c):
    return (p[0] * c * c % P, p[1] * c ** 3 % P)


def _cofactors(zs):
    """product of the others, by prefix / suffix products (no inversion)"""
    n = len(zs)
    pre, suf = [1] * (n + 1), [1] * (n + 1)
    for i in range(n):
        pre[i + 1] = pre[i] * zs[i] % P
    for i in range(n - 1, -1, -1):
        suf[i] = suf[i + 1] * zs[i] % P
    return [pre[i] * suf[i + 1] % P for i in range(n)], pre[n]


def _double_n(pt, n):
    """n Jacobian doublings by jacobian29.h's formulas, on values"""
    x, y, z = pt
    half = pow(2, -1, P)
    for _ in range(n):
        l = 3 * x * x * half % P
        s = y * y % P
        t = -x * s % P
        x3 = (l * l + 2 * t) % P
        y3 = -(l * (x3 + t) + s * s) % P
        x, y, z = x3, y3, y * z % P
    return x, y, z


def chain_comb(Q):
    """k_key_chain<false, KC_TEETH> with kc_sets on values: the lead pair (x, y, x, y, z) and what it leaves for k_key_finish_comb: twelve points
    A_0 .. A_3, C_0 .. C_7 over Z_AC, and Z_AC"""
    cur = (Q[0], Q[1], 1)
    bases = [cur]
    for _ in range(1, TEETH):
        cur = _double_n(cur, SPACING)
        bases.append(cur)
    lx, ly, lz = _double_n(cur, 1)
    (sx, sy), (dx, dy), h = _conj((lx, ly), (lx * R.BETA % P, ly))
    lead = ((sx, sy), (dx, dy), lz * h % P)
    co, zb = _cofactors([b[2] for b in bases])
    b = [_rescale((bases[t][0], bases[t][1]), co[t]) for t in range(TEETH)]
    pt, f = [None] * 12, [None] * 6
    s, d, h1 = _conj(b[6], b[5])
    b4 = _rescale(b[4], h1)
    pt[0], pt[1], h2 = _conj(s, b4)
    pt[2], pt[3], h3 = _conj(d, b4)
    f[0], f[1] = h1 * h2 % P, h1 * h3 % P
    s1, d1, g1 = _conj(b[3], b[2])
    s2, d2, g2 = _conj(b[1], b[0])
    s1, d1, s2, d2 = _rescale(s1, g2), _rescale(d1, g2), _rescale(s2, g1), _rescale(d2, g1)
    for k, (u, v) in enumerate(((s1, s2), (s1, d2), (d1, s2), (d1, d2))):
        pt[4 + 2 * k], pt[5 + 2 * k], hk = _conj(u, v)
        f[2 + k] = g1 * g2 * hk % P
    cf, fall = _cofactors(f)
    pt = [_rescale(pt[n], cf[n // 2]) for n in range(12)]
    return lead, pt, zb * fall % P


KC_CBITS = _const("KC_CBITS", "keyed.hip")


def kc_entry(i, j, minus):
    cb = (KC_CBITS >> (4 * j)) & 7
    return ((3 - i) << 4) | ((7 - cb) if minus else (8 | cb))


def finish_comb(lead, pt, zac):
    """k_key_finish_comb on values, the eight lanes of one key: entries[idx] = (x, y, beta x), the lead pair, W"""
    (ls, ld, zl) = lead
    entries, hs = {}, []
    for j in range(8):
        lane = []
        for i in range(4):
            s, d, h = _conj(pt[i], pt[4 + j])
            entries[kc_entry(i, j, False)] = s
            entries[kc_entry(i, j, True)] = d
            lane.append(h)
        hs.append(lane)
    pj = [h[0] * h[1] * h[2] * h[3] % P for h in hs]
    others, allp = _cofactors([zl] + pj)                           # lane j: the lead pair's Z and the other lanes' products
    for j in range(8):
        e, _ = _cofactors(hs[j])
        for i in range(4):
            q = others[1 + j] * e[i] % P
            for minus in (False, True):
                x, y = _rescale(entries[kc_entry(i, j, minus)], q)
                entries[kc_entry(i, j, minus)] = (x, y, x * R.BETA % P)
    co = allp * pow(zl, -1, P) * zac % P                           # (the kernel: suf * pj * zac in lane 0)
    return entries, (_rescale(ls, co), _rescale(ld, co)), co * zl % P


def test_index_constants():
    assert sorted(kc_entry(i, j, mi) for i in range(4) for j in range(8) for mi in (False, True)) == list(range(64))
    assert re.search(r"return \(\(3u - i\) << 4\) \| \(minus \? 7u - cb : 8u \| cb\);", fm.source("keyed.hip"))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_build_gives_every_entry(seed):
    rng = random.Random(9100 + seed)
    d = rng.randrange(1, N)
    Q = R.mul(d, R.G)
    lead, pt, zac = chain_comb(Q)
    # the A and C sets over one Z
    for i, (s5, s4) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
        k = (1 << (6 * SPACING)) + s5 * (1 << (5 * SPACING)) + s4 * (1 << (4 * SPACING))
        assert _affine(pt[i][0], pt[i][1], zac) == R.mul(k * d % N, R.G), i
    for j in range(8):
        cb = (KC_CBITS >> (4 * j)) & 7
        k = (1 << (3 * SPACING)) + sum((2 * ((cb >> t) & 1) - 1) << (SPACING * t) for t in range(3))
        assert _affine(pt[4 + j][0], pt[4 + j][1], zac) == R.mul(k * d % N, R.G), j
    entries, (ls, ld), W = finish_comb(lead, pt, zac)
    assert sorted(entries) == list(range(64))
    for idx, (x, y, bx) in entries.items():
        assert _affine(x, y, W) == R.mul(entry_scalar(idx) * d % N, R.G), idx
        assert bx == x * R.BETA % P
    L = (1 << LEAD_LOG2) * d % N
    assert _affine(ls[0], ls[1], W) == R.mul(L * (1 + R.LAMBDA) % N, R.G)
    assert _affine(ld[0], ld[1], W) == R.mul(L * (1 - R.LAMBDA) % N, R.G)


def test_ladder_over_the_built_table():
    """the whole path on values for a few scalars, boundary halves among them: lead, 19 rounds, the factor W"""
    import test_glv_odd_model as glv
    rng = random.Random(77)
    d = rng.randrange(1, N)
    Q = R.mul(d, R.G)
    lead, pt, zac = chain_comb(Q)
    entries, (ls, ld), W = finish_comb(lead, pt, zac)

    def aff(x, y):
        return _affine(x, y, W)

    for u2 in [1, 2, 3, R.LAMBDA, R.LAMBDA + 1, N - 1, (N + 1) // 2, 2**128 + 1] + [rng.randrange(1, N) for _ in range(6)]:
        k1, k2 = glv.make_odd(*glv.split_reference(u2))
        n1, n2 = k1 < 0, k2 < 0
        x, y = ls if n1 == n2 else ld
        acc = aff(x, -y % P if n1 else y)
        d1, d2 = comb_digits(abs(k1)), comb_digits(abs(k2))
        for r in range(SPACING):
            if r:
                acc = R.add(acc, acc)
            for half, (entry, negative) in enumerate((d1[r], d2[r])):
                x, y, bx = entries[entry]
                if negative != (n2 if half else n1):
                    y = -y % P
                acc = R.add(acc, aff(bx if half else x, y))
        assert acc == R.mul(u2, Q), hex(u2)


# ==== the kernels' call sequences: bounds and drift guard ================================================================
@cpp("kc_sets")
def kc_sets(bx, by, z):
    """the calls in text order, every loop's body once (the unrolled loops: one trip with every branch); a base as k_key_chain
    parks it: x [1], y [<= 2], z [1]"""
    pre = mul(z, z)
    co = mul(pre, z)
    suf = mul(z, z)
    c2 = sqr(co)
    b = coz_rescale((bx, by), c2, mul(c2, co))
    s, d, h1 = coz_conj(b, b)
    h1_2 = sqr(h1)
    b4 = coz_rescale(b, h1_2, mul(h1_2, h1))
    p0, p1, h2 = coz_conj(s, b4)
    p2, p3, h3 = coz_conj(d, b4)
    f0 = mul(h1, h2)
    f1 = mul(h1, h3)
    s1, d1, g1 = coz_conj(b, b)
    s2, d2, g2 = coz_conj(b, b)
    g1_2 = sqr(g1)
    g1_3 = mul(g1_2, g1)
    g2_2 = sqr(g2)
    g2_3 = mul(g2_2, g2)
    s1 = coz_rescale(s1, g2_2, g2_3)
    d1 = coz_rescale(d1, g2_2, g2_3)
    s2 = coz_rescale(s2, g1_2, g1_3)
    d2 = coz_rescale(d2, g1_2, g1_3)
    gg = mul(g1, g2)
    fs = [f0, f1]
    pts = [p0, p1, p2, p3]
    for u, v in ((s1, s2), (s1, d2), (d1, s2), (d1, d2)):
        a_, b_, hk = coz_conj(u, v)
        fs.append(mul(gg, hk))
        pts += [a_, b_]
    pf = mul(fs[0], fs[1])
    zac = mul(pre, pf)
    co = mul(pf, fs[5])
    suf = mul(fs[5], fs[4])
    c2 = sqr(co)
    c3 = mul(c2, co)
    u = coz_rescale(pts[0], c2, c3)
    v = coz_rescale(pts[1], c2, c3)
    return (u, v), zac, pts, (pre, suf)


@cpp("k_key_finish_comb")
def key_finish_comb(a, c, zl, zac, lead):
    lx, ly, dx, dy = lead
    s, d, h = coz_conj(a, c)
    h01 = mul(h, h)
    h23 = mul(h, h)
    e = [mul(h, h23), mul(h, h23), mul(h01, h), mul(h01, h)]
    pj = mul(h01, h23)
    pre = select(group_shr(pj), zl)
    pre = mul(pre, group_shr(pre))
    pre = mul(pre, group_shr(pre))
    pre = mul(pre, group_shr(pre))
    suf = group_shl(pj)
    suf = mul(suf, group_shl(suf))
    suf = mul(suf, group_shl(suf))
    suf = mul(suf, group_shl(suf))
    rr = mul(pre, suf)
    co = mul(mul(suf, pj), zac)
    beta = from_words()
    q = mul(rr, e[0])
    q2 = sqr(q)
    q3 = mul(q2, q)
    s = coz_rescale(s, q2, q3)
    d = coz_rescale(d, q2, q3)
    outs = [s[0], s[1], mul(s[0], beta), d[0], d[1], mul(d[0], beta)]
    outs.append(mul(co, zl))
    s2 = sqr(co)
    s3 = mul(s2, co)
    outs += [mul(lx, s2), mul(ly, s3), zero(), mul(dx, s2), mul(dy, s3), zero()]
    return outs


LEAD4 = (NW, PROD, NW, PROD)               # the lead pair's x, y, x, y as kt_store_lead_pair leaves them


def test_sets_bounds():
    # the bases are jpt29 points of the doubling chain (test_fe29_formulas_model.key_chain: x [1], y [<= 2], z [1])
    (u, v), zac, pts, prods = kc_sets(COORD, Y2, COORD)
    assert within(u, APT) and within(v, APT) and le(zac, COORD) and all(within(p, APT) for p in pts) and all(le(x, COORD) for x in prods)


def test_finish_comb_bounds():
    outs = key_finish_comb(APT, APT, COORD, COORD, LEAD4)
    assert all(le(o, COORD) for o in outs), "a stored value is above 1 unit"


@pytest.fixture
def tracked(monkeypatch):
    monkeypatch.setattr(fm, "TRACKED", re.compile(fm.TRACKED.pattern.replace(r"(fe29_\w+", r"(fe29_\w+|coz29_\w+")))


GUARDED = [
    (coz_conj, (APT, APT), "keyed.hip", "coz29_conj"),
    (coz_rescale, (APT, COORD, COORD), "keyed.hip", "coz29_rescale"),
    (kc_sets, (COORD, Y2, COORD), "keyed.hip", "kc_sets"),
    (key_finish_comb, (APT, APT, COORD, COORD, LEAD4), "keyed.hip", "k_key_finish_comb"),
]


@pytest.mark.parametrize("g", GUARDED, ids=[g[3] for g in GUARDED])
def test_drift_guard(g, tracked):
    fn, args, fname, func = g
    assert m.record(fn, *args) == fm.calls_in(fm.body_of(fname, func)), f"{func} ({fname}) no longer matches its model"


MUTATIONS = [
    ("coz29_conj: fe29_negate(p.x, 1) -> 0", coz_conj, (APT, APT), ("fe29_negate", 0, fm._lower)),
    ("coz29_conj: drop fe29_normalize_weak of h", coz_conj, (APT, APT), ("fe29_normalize_weak", 0, None)),
    ("coz29_conj: drop fe29_normalize_weak of Y_Q - Y_P", coz_conj, (APT, APT), ("fe29_normalize_weak", 1, None)),
    ("coz29_conj: drop fe29_normalize_weak of -Y_Q - Y_P", coz_conj, (APT, APT), ("fe29_normalize_weak", 2, None)),
    ("coz29_conj: fe29_negate(fe29_add(b, c), 2) -> 1", coz_conj, (APT, APT), ("fe29_negate", 1, fm._lower)),
]


@pytest.mark.parametrize("mu", MUTATIONS, ids=[mu[0] for mu in MUTATIONS])
def test_mutation_is_rejected(mu):
    _, fn, args, mutation = mu
    fn(*args)
    with pytest.raises(AssertionError):
        m.mutated(fn, mutation, *args)


def test_the_ladder_runs_19_rounds_of_two_additions():
    body = fm.body_of("verify_fast.h", "k_verify_fast")
    comb = body[body.index("if constexpr (COMB) {"):body.index("} else if constexpr (KEYED) {")]
    assert comb.count("jpt29_add_affine(") == 1 and comb.count("jpt29_double(") == 1
    assert "for (int j = G::SPACING - 1;; --j)" in comb and "if (j == 0) break;" in comb
    assert comb.index("jpt29_add_affine(") < comb.index("if (j == 0) break;") < comb.index("jpt29_double(")


def test_chosen_u2_of_the_device_test_reach_the_small_boundary_halves():
    """which boundary halves the device's split can produce at all, for the u2 of tests/test_gpu_comb.py: |k| = 1 and 3 come
    out of it; halves of 2^128 and more do not (the split returns the short representative), so those are covered on
    integers above and on the device only as values of u2"""
    import test_glv_odd_model as glv
    import test_gpu_comb as gc
    halves = set()
    for u2 in gc.chosen_u2():
        halves |= {abs(k) for k in glv.make_odd(*glv.split_reference(u2))}
    assert {1, 3} <= halves
    assert max(halves) < 1 << 129 and all(k & 1 for k in halves)
    assert len(gc.chosen_u2()) * 16 <= gc.NSIG // 2 + 2 * len(gc.chosen_u2())     # every u2 meets several keys in the valid half
