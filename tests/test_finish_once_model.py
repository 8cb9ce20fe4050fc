"""Model of k_key_finish_comb_once (keyed.hip): the comb table's finish kernel with the cofactors formed FIRST - the four
h_i = X(C_j) - X(A_i) of a lane are subtractions of values that are in memory when the kernel starts, so e_i, the lane's
product, the prefix / suffix products over the key's eight lanes, rr and co come before any addition, and every pair is
added, scaled and stored once.  Without a GPU:

  * interval bounds over the kernel's own call sequence (drift-guarded against the C++ body), the h formed outside
    coz29_conj against the one formed inside;
  * both orders of operations on LIMBS for whole keys, the eight lanes with their row_shr / row_shl products as the kernels
    run them: k_key_finish_comb (add, park, cofactors, fetch, scale) and k_key_finish_comb_once give the same 64 entries,
    lead pair and W limb for limb, which are finish_comb's values and the affine points entry_scalar(idx) Q scaled by W;
  * the source: no park, no fetch and no `back` offset in the new kernel; the old one keeps them (it is the A/B reference).
"""
import random

import pytest

import pyref as R
import test_comb_model as cm
import test_fe29_formulas_model as fm
import test_fe29_model as m
from test_comb_model import APT, LEAD4, chain_comb, coz_conj, coz_rescale, finish_comb, kc_entry, tracked  # noqa: F401  (tracked: fixture)
from test_coz_model import group_shr
from test_fe29_formulas_model import COORD, from_words, group_shl, le, select, zero
from test_fe29_model import P, add, cpp, mul, negate, normalize_weak, sqr

N = R.N


# ==== the kernel's call sequence: bounds and drift guard =================================================================
@cpp("k_key_finish_comb_once")
def key_finish_comb_once(a, c, zl, zac, lead):
    """the calls in text order, every loop's body once; returns what the kernel stores, and the two h"""
    lx, ly, dx, dy = lead
    h = normalize_weak(add(c[0], negate(a[0], 1)))
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
    s, d, h_in = coz_conj(a, c)
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
    return outs, h, h_in


ARGS = (APT, APT, COORD, COORD, LEAD4)


def test_finish_once_bounds():
    outs, h, h_in = key_finish_comb_once(*ARGS)
    assert len(outs) == 13 and all(le(o, COORD) for o in outs), "a stored value is above 1 unit"
    assert h.hi == h_in.hi and le(h, COORD), "the h formed outside coz29_conj is not bounded as the one formed inside"
    # the same stores, under the same bounds, as the kernel that parks
    assert [o.hi for o in outs] == [o.hi for o in cm.key_finish_comb(*ARGS)]


def test_finish_once_drift_guard(tracked):
    assert m.record(key_finish_comb_once, *ARGS) == fm.calls_in(fm.body_of("keyed.hip", "k_key_finish_comb_once")), \
        "k_key_finish_comb_once (keyed.hip) no longer matches its model"


def test_h_is_the_expression_of_coz29_conj():
    """the text of the subtraction, operands aside: what coz29_conj does for its h the new kernel does for its own"""
    import re
    conj = fm.body_of("keyed.hip", "coz29_conj")
    once = fm.body_of("keyed.hip", "k_key_finish_comb_once")
    assert "fe29_normalize_weak(fe29_add(q.x, fe29_negate(p.x, 1)))" in conj
    assert re.search(r"fe29_normalize_weak\(fe29_add\(c\.x, fe29_negate\(ke_load\(ka \+ \(size_t\)i \* 8, TB_X\), 1\)\)\)", once)
    assert "coz29_conj(a, c, s, d)" in once                    # p = A_i, q = C_j: h = X_C - X_A in both places


# ==== the source =========================================================================================================
def test_source_no_park_in_the_new_kernel():
    once = fm.body_of("keyed.hip", "k_key_finish_comb_once")
    park = fm.body_of("keyed.hip", "k_key_finish_comb")
    for word in ("ke_store_xy", "ke_fetch_xy", "back"):
        assert word not in once, word
        assert word in park, f"k_key_finish_comb lost its {word}: it is the A/B reference"
    assert once.count("ke_store3(") == 4 and once.count("ke_store(") == 1      # two per pair in the loop, the lead pair; W
    assert "#pragma unroll 1\n  for (int i = 3; i >= 0; --i)" in once


def test_the_knob_is_read_at_every_call():
    body = fm.body_of("keyed.hip", "s2k_internal_key_tables")
    assert 'const char* fin = getenv("S2K_KEY_FINISH_COMB");' in body and "static const char* fin" not in body
    assert 'strcmp(fin, "park") == 0' in body
    assert body.count("k_key_finish_comb<<<") == 1 and body.count("k_key_finish_comb_once<<<") == 1


# ==== both orders on limbs ===============================================================================================
BETA_LIMBS = m.from_int(R.BETA)
ONE = m.from_int(1)


def _mul(a, b):
    return m.mulsum_int([(a, b)])


def _rescale_int(p, c2, c3):
    return (_mul(p[0], c2), _mul(p[1], c3))


def _shr(v, n, keep):
    """fe29_group_shr<n> over the eight lanes: lane j reads lane j - n; keep[j] false: one"""
    return [v[j - n] if keep[j] else ONE for j in range(8)]


def _shl(v, n, keep):
    return [v[j + n] if keep[j] else ONE for j in range(8)]


def _across_lanes(pj, zl, zac):
    """rr and co of the eight lanes from their products pj, as both kernels form them"""
    lanes = range(8)
    pre = _shr(pj, 1, [j > 0 for j in lanes])
    pre = [zl if j == 0 else pre[j] for j in lanes]
    for n, keep in ((1, [j > 0 for j in lanes]), (2, [j > 1 for j in lanes]), (4, [j > 3 for j in lanes])):
        sh = _shr(pre, n, keep)
        pre = [_mul(pre[j], sh[j]) for j in lanes]
    suf = _shl(pj, 1, [j < 7 for j in lanes])
    for n, keep in ((1, [j < 7 for j in lanes]), (2, [j < 6 for j in lanes]), (4, [j < 4 for j in lanes])):
        sh = _shl(suf, n, keep)
        suf = [_mul(suf[j], sh[j]) for j in lanes]
    rr = [_mul(pre[j], suf[j]) for j in lanes]
    co = [_mul(_mul(suf[j], pj[j]), zac) for j in lanes]
    return rr, co


def _in_lane(h):
    h01, h23 = _mul(h[0], h[1]), _mul(h[2], h[3])
    e = [_mul(h[1], h23), _mul(h[0], h23), _mul(h01, h[3]), _mul(h01, h[2])]
    return e, _mul(h01, h23)


def _entry3(p):
    return (p[0], p[1], _mul(p[0], BETA_LIMBS))


def _lead_and_w(co0, zl, ls, ld):
    s2 = _mul(co0, co0)
    s3 = _mul(s2, co0)
    return (_rescale_int(ls, s2, s3), _rescale_int(ld, s2, s3)), _mul(co0, zl)


def finish_park_int(A, C, zl, zac, ls, ld):
    """k_key_finish_comb: add and park, cofactors, fetch back, scale.  Returns (entries, writes per entry, lead pair, W)"""
    mem, writes = {}, {}
    hs = []
    for j in range(8):
        lane = []
        for i in range(4):
            s, d, h = cm.conj_int(A[i], C[j])
            for minus, p in ((False, s), (True, d)):
                mem[kc_entry(i, j, minus)] = p                  # ke_store_xy: raw limbs
            lane.append(h)
        hs.append(lane)
    es, pj = zip(*(_in_lane(h) for h in hs))
    rr, co = _across_lanes(list(pj), zl, zac)
    for j in range(8):
        for i in (3, 2, 1, 0):
            q = _mul(rr[j], es[j][i])
            q2 = _mul(q, q)
            q3 = _mul(q2, q)
            for minus in (False, True):
                idx = kc_entry(i, j, minus)
                mem[idx] = _entry3(_rescale_int(mem[idx], q2, q3))
                writes[idx] = writes.get(idx, 0) + 1
    return (mem, writes) + _lead_and_w(co[0], zl, ls, ld)


def finish_once_int(A, C, zl, zac, ls, ld):
    """k_key_finish_comb_once: the h by subtraction, cofactors, then each pair added, scaled and stored"""
    mem, writes = {}, {}
    hs = [[m.normalize_weak_int([x + y for x, y in zip(C[j][0], m.negate_int(A[i][0], 1))]) for i in range(4)] for j in range(8)]
    es, pj = zip(*(_in_lane(h) for h in hs))
    rr, co = _across_lanes(list(pj), zl, zac)
    for j in range(8):
        for i in (3, 2, 1, 0):
            s, d, h = cm.conj_int(A[i], C[j])
            assert h == hs[j][i], "coz29_conj recomputes another h than the one the cofactors were made of"
            q = _mul(rr[j], es[j][i])
            q2 = _mul(q, q)
            q3 = _mul(q2, q)
            for minus, p in ((False, s), (True, d)):
                idx = kc_entry(i, j, minus)
                assert idx not in mem
                mem[idx] = _entry3(_rescale_int(p, q2, q3))
                writes[idx] = writes.get(idx, 0) + 1
    return (mem, writes) + _lead_and_w(co[0], zl, ls, ld)


def _lazy(rng, v):
    """a value as a product leaves it: some representative of v below 2^256 + a little, limbs [<= 1 unit]"""
    return m.from_int(v + P * rng.randrange(2) if v + P < 1 << 256 else v)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_both_orders_give_the_same_table(seed):
    rng = random.Random(12000 + seed)
    d = rng.randrange(1, N)
    Q = R.mul(d, R.G)
    (ls_v, ld_v, zl_v), pt_v, zac_v = chain_comb(Q)
    pt = [(_lazy(rng, x), _lazy(rng, y)) for x, y in pt_v]
    A, C = pt[:4], pt[4:]
    zl, zac = _lazy(rng, zl_v), _lazy(rng, zac_v)
    ls, ld = tuple(_lazy(rng, v) for v in ls_v), tuple(_lazy(rng, v) for v in ld_v)
    park = finish_park_int(A, C, zl, zac, ls, ld)
    once = finish_once_int(A, C, zl, zac, ls, ld)
    # limb for limb
    assert sorted(once[0]) == list(range(64))
    assert once[0] == park[0] and once[2] == park[2] and once[3] == park[3]
    assert all(n == 1 for n in once[1].values()) and len(once[1]) == 64, "an entry is not written exactly once"
    assert all(x <= m.M + (1 << 20) for e in once[0].values() for v in e for x in v)
    # the values: finish_comb's, and the affine points of the comb scaled by W
    entries, (ls_w, ld_w), W = finish_comb((ls_v, ld_v, zl_v), pt_v, zac_v)
    val = lambda v: m.value(v) % P
    assert val(once[3]) == W
    assert tuple(tuple(val(v) for v in p) for p in once[2]) == (ls_w, ld_w)
    for idx in range(64):
        x, y, bx = (val(v) for v in once[0][idx])
        assert (x, y, bx) == entries[idx], idx
        assert cm._affine(x, y, W) == R.mul(cm.entry_scalar(idx) * d % N, R.G), idx
        ax, ay = cm._affine(x, y, W)
        assert (ay * ay - ax * ax * ax - 7) % P == 0 and bx == x * R.BETA % P
