"""Point sets (s2k_pointset_*) on the GPU, at both digit widths: the stored tables against the oracle's multiples, and every
segment's record against the CPU oracle (Straus per segment on the expanded point list, reduced scalars), never against the
engine's own segmented call alone."""
import ctypes as C
import random

import numpy as np
import pytest

import pointset_model as M
import pyref as R
from pyref import b32

pytestmark = pytest.mark.gpu
IDENT = bytes(65)
ERR_ARG, ERR_NOMEM = -3, -4
WIDTHS = [4, 8]
T = 8                                 # S2K_POINTSET_T, the default piece length (pointset.hip)


@pytest.fixture(scope="module")
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def pool(oracle):
    """300 points of known discrete logarithm."""
    rnd = random.Random(9001)
    d = [rnd.randrange(1, R.N) for _ in range(300)]
    return d, [oracle.scalar_base_mult_vartime(b32(x)) for x in d]


@pytest.fixture(scope="module")
def sets(eng, pool):
    """Point sets over the first m points of the pool, made once per (width, m)."""
    made = {}

    def get(c, m):
        if (c, m) not in made:
            made[(c, m)] = eng.pointset_create(pool[1][:m], c)
            assert len(made[(c, m)]) == m and made[(c, m)].window_bits() == c
        return made[(c, m)]
    yield get
    for ps in made.values():
        ps.close()


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def expect_segments(oracle, ks, ps, lens):
    out, a = [], 0
    for L in lens:
        kr = [oracle.fn_reduce(k)[0] for k in ks[a:a + L]]
        out.append(oracle.multi_scalar_mult_vartime(kr, ps[a:a + L]) if L else IDENT)
        a += L
    return out


def dense_points(pts, lens):
    return [pts[t] for L in lens for t in range(L)]


def run(ps, ks, lens, idx=None):
    got = ps.multi_scalar_mult_segments(ks, offsets_of(lens), idx)
    assert got.shape == (len(lens), 65)
    return [bytes(r) for r in got]


def rand_scalars(rnd, count):
    return [b32(rnd.randrange(R.N)) for _ in range(count)]


# ---- 1. the tables -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WIDTHS)
def test_table_entries(eng, oracle, pool, c):
    import secp256k1_voi_amd as S
    d, pts = pool
    positions, entries, nbytes = S.pointset_geometry(c)
    ps = eng.pointset_create(pts[:3] + [IDENT], c)
    try:
        assert ps.device_bytes() >= 4 * nbytes
        wanted = {(pos, mag) for pos in range(positions) for mag in (1, 2, 3, entries - 1, entries)}
        wanted |= {(pos, mag) for pos in (0, 1) for mag in range(1, entries + 1)}
        for pos, mag in sorted(wanted):
            for i in range(3):
                exp = oracle.scalar_base_mult_vartime(b32(d[i] * mag * (1 << (c * pos)) % R.N))
                assert ps.entry(i, pos, mag) == exp[1:], (i, pos, mag)
            assert ps.entry(3, pos, mag) == bytes(64)                  # the identity record has no table
        lib = eng._lib
        buf = np.zeros(64, dtype=np.uint8)
        for i, pos, mag in ((4, 0, 1), (0, positions, 1), (0, 0, 0), (0, 0, entries + 1)):
            assert lib.s2k_debug_pointset_entry(ps._k, i, pos, mag, buf.ctypes.data) == ERR_ARG
    finally:
        ps.close()


# ---- 2. dense shapes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seg", [1, 2, 63, 64, 65, 300])
@pytest.mark.parametrize("c", WIDTHS)
def test_dense_shapes(oracle, pool, sets, c, n_seg):
    rnd = random.Random(100 * c + n_seg)
    pts = pool[1]
    for m in (1, 2, 7, 8, 9, 64, 65):
        ps = sets(c, m)
        if n_seg == 1:
            shapes = [[m], [m - 1], [0]]
        elif n_seg == 2:
            shapes = [[m, 0], [0, m], [m // 2, m]]
        else:
            lens = [m, m - 1, m // 2] + [rnd.randrange(0, m + 1) for _ in range(n_seg - 12)]
            rnd.shuffle(lens)
            mid = len(lens) // 2
            lens = [0, 0, 0] + lens[:mid] + [0, 0, 0] + lens[mid:] + [0, 0, 0]      # empty segments: start, middle, end
            assert len(lens) == n_seg
            shapes = [lens]
        for lens in shapes:
            ks = rand_scalars(rnd, sum(lens))
            assert run(ps, ks, lens) == expect_segments(oracle, ks, dense_points(pts, lens), lens), (m, lens[:20])
        # no terms at all: identity records, and no segments: nothing
        got = ps.multi_scalar_mult_segments([], np.zeros(n_seg + 1, dtype=np.uint64))
        assert got.shape == (n_seg, 65) and not got.any()
    assert sets(c, 7).multi_scalar_mult_segments([], [0]).shape == (0, 65)


# ---- 3. indexed shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WIDTHS)
def test_indexed_shapes(oracle, pool, sets, c):
    rnd = random.Random(300 + c)
    pts, ps = pool[1], sets(c, 16)
    lens = [0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 63, 64, 65, 255, 300]
    lens += [rnd.choice([0, 1, 2, 3, T - 1, T, T + 1, 2 * T + 1]) for _ in range(40)]
    rnd.shuffle(lens)
    idx = [rnd.randrange(16) for _ in range(sum(lens))]
    # the same index 40 times in one segment; and one point on both sides of a piece border, several times
    lens += [40, 2 * T + 3]
    idx += [5] * 40
    idx += [rnd.randrange(16) for _ in range(T - 2)] + [9, 9, 9, 9] + [rnd.randrange(16) for _ in range(T + 1)]
    lens = [0] + lens + [0]
    ks = rand_scalars(rnd, sum(lens))
    assert len(idx) == len(ks)
    assert run(ps, ks, lens, idx) == expect_segments(oracle, ks, [pts[i] for i in idx], lens)


# ---- 4. the edge pool of the segmented call's tests, in four placements ------------------------------------------------------
def edge_cases(oracle, eng, pts, c, rnd):
    """The set: P, -P, a second copy of P, lambda P, an identity record, then seven more points.  Cases: (scalars, indices)."""
    P = pts[0]
    lamP = b"\x04" + b32(R.BETA * int.from_bytes(P[1:33], "big") % R.P) + P[33:]
    members = [P, oracle.point_neg(P), P, lamP, IDENT] + pts[1:8]
    k2 = rnd.randrange(1, R.N)
    small = [int.from_bytes(b"\x80" * 15, "big"), int.from_bytes(b"\x7f" * 16, "big"), 0x80]
    for k in small:                                       # below 2^127 the half scalar is the scalar itself
        assert k < 1 << 127 and M.split(k) == (k, False, 0, False)
    carry = next(k for k in (rnd.randrange(R.N) for _ in range(10000)) if M.reaches_carry(k, c))
    m1, _, m2, _ = M.split(carry)
    assert M.recode(m1, c)[-1] == 1 or M.recode(m2, c)[-1] == 1
    h1, h2 = eng.fn_split_glv_batch([b32(carry)])         # the engine's own split has the same two magnitudes
    mags = [min(v, R.N - v) for v in (int.from_bytes(bytes(h1[0]), "big"), int.from_bytes(bytes(h2[0]), "big"))]
    assert mags == [m1, m2]
    cases = [
        ([5] * 40, [0] * 40),                                           # the same point 40 times
        ([7, 7], [0, 1]),                                               # P and -P: identity
        ([1, R.N - 1], [5, 5]),                                         # k and n - k on one point: identity
        ([0] * 5, [0, 1, 2, 3, 5]),                                     # zero scalars
        ([3, 4], [4, 6]),                                               # an identity record
        ([0, R.N - 1, R.N, R.N + 1, 2**256 - 1], [5, 6, 7, 8, 9]),      # reduced as SetBytes does
        ([sum(0xFFFF << (16 * i) for i in range(0, 16, 2)), 1 << 255], [8, 9]),
        ([1 << 128, (1 << 128) - 1], [10, 11]),
        ([(R.N - k2 * R.LAMBDA) % R.N, k2], [0, 3]),                    # P and lambda P, scalars that cancel
        ([2, R.N - 1, R.N - 1], [0, 2, 0]),                             # P + P (its second copy) inside the sum, then identity
        (small, [5, 0, 3]),
        ([carry, carry], [0, 6]),                                       # a half scalar with the carry digit
        ([k2, R.N - k2], [7, 7]),                                       # k with n - k
    ]
    cases = [([b32(k) for k in ks], ix) for ks, ix in cases]
    pm = [members[i] for i in cases[8][1]]
    assert oracle.multi_scalar_mult_vartime(cases[8][0], pm) == IDENT          # the cancelling pair
    return members, cases


@pytest.mark.parametrize("c", WIDTHS)
def test_edge_pool_placements(eng, oracle, pool, c):
    rnd = random.Random(61 + c)
    members, cases = edge_cases(oracle, eng, pool[1], c, rnd)
    ps = eng.pointset_create(members, c)
    m = len(members)

    def terms(count):
        return rand_scalars(rnd, count), [rnd.randrange(m) for _ in range(count)]

    def check(ks, ix, lens):
        assert run(ps, ks, lens, ix) == expect_segments(oracle, ks, [members[i] for i in ix], lens), lens[:10]
    try:
        for ck, ci in cases:
            ak, ai = terms(3)
            bk, bi = terms(T + 2)
            check(ak + ck + bk, ai + ci + bi, [3, len(ck), T + 2])                        # (a) a segment of its own
            check(ak + ck + bk, ai + ci + bi, [3, len(ck) + T + 2])                       # (b) at the start of a segment
            check(bk[:T - 1] + ck + ak, bi[:T - 1] + ci + ai, [T - 1 + len(ck) + 3])      # (c) across a piece border
        # (d) every case as a segment among 1000 random ones: the neighbours' results must not change
        lens = [rnd.randrange(0, 5) for _ in range(1000)]
        ks, ix = terms(sum(lens))
        base = expect_segments(oracle, ks, [members[i] for i in ix], lens)
        assert run(ps, ks, lens, ix) == base
        offs = [0]
        for L in lens:
            offs.append(offs[-1] + L)
        where = sorted(rnd.sample(range(1001), len(cases)), reverse=True)
        lens2, ks2, ix2, exp2 = list(lens), list(ks), list(ix), list(base)
        for (ck, ci), at in zip(cases, where):            # back to front: earlier positions stay valid
            t = offs[at]
            lens2.insert(at, len(ck))
            ks2[t:t] = ck
            ix2[t:t] = ci
            exp2.insert(at, oracle.multi_scalar_mult_vartime([oracle.fn_reduce(k)[0] for k in ck], [members[i] for i in ci]))
        assert run(ps, ks2, lens2, ix2) == exp2
    finally:
        ps.close()


# ---- 5. the same record as the segmented call ----------------------------------------------------------------------------
@pytest.mark.parametrize("c", WIDTHS)
def test_equals_segmented_call(eng, pool, sets, c):
    rnd = random.Random(500 + c)
    pts, ps = pool[1], sets(c, 16)
    lens = [rnd.randrange(0, 41) for _ in range(300)]
    ks = rand_scalars(rnd, sum(lens))
    idx = [rnd.randrange(16) for _ in range(sum(lens))]
    want = eng.multi_scalar_mult_segments(ks, [pts[i] for i in idx], offsets_of(lens))
    assert np.array_equal(ps.multi_scalar_mult_segments(ks, offsets_of(lens), idx), want)


# ---- 6. long segments: gathered from the set, then the bucket method -------------------------------------------------------
@pytest.mark.parametrize("c", WIDTHS)
def test_long_segment_route(oracle, pool, sets, c, monkeypatch):
    monkeypatch.setenv("S2K_POINTSET_CROSSOVER", "16")     # (read at every call)
    rnd = random.Random(600 + c)
    pts = pool[1]
    lens = [17, 3, 0, 64, 16, 300, 0, 8, 17, 0]
    ks = rand_scalars(rnd, sum(lens))
    idx = [rnd.randrange(16) for _ in range(sum(lens))]
    assert run(sets(c, 16), ks, lens, idx) == expect_segments(oracle, ks, [pts[i] for i in idx], lens)
    assert run(sets(c, 300), ks, lens) == expect_segments(oracle, ks, dense_points(pts, lens), lens)
    one = [300]                                            # one long segment alone
    assert run(sets(c, 300), ks[:300], one) == expect_segments(oracle, ks[:300], dense_points(pts, one), one)


# ---- 7. the device form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", WIDTHS)
def test_device_form_behind_hash_to_curve(eng, oracle, c):
    import torch
    import secp256k1_voi_amd as S
    rnd = random.Random(700 + c)
    dev = torch.device("cuda", 0)
    m = 24
    msgs = np.frombuffer(rnd.randbytes(m * 32), dtype=np.uint8).copy()
    d_msgs = torch.from_numpy(msgs).to(dev)
    d_rec = torch.zeros(m * 65, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.hash_to_curve_device(S.H2C_SSWU_RO, m, b"pointset-test-secp256k1_XMD:SHA-256_SSWU_RO_", d_msgs.data_ptr(), None, 32, m * 32,
                             d_rec.data_ptr(), stream.cuda_stream)
    recs = d_rec.cpu().numpy().reshape(m, 65)              # the set's input records: what the device hashed
    members = [bytes(r) for r in recs]
    ps = eng.pointset_create(recs, c)
    try:
        lens = [0, 5, T, 0, 2 * T + 1, 40, 1, 0]
        n = sum(lens)
        ks = rand_scalars(rnd, n)
        idx = [rnd.randrange(m) for _ in range(n)]
        off = offsets_of(lens)
        host = ps.multi_scalar_mult_segments(ks, off, idx)
        assert [bytes(r) for r in host] == expect_segments(oracle, ks, [members[i] for i in idx], lens)
        with torch.cuda.stream(stream):
            dk = torch.from_numpy(np.frombuffer(b"".join(ks), dtype=np.uint8).copy()).to(dev)
            di = torch.from_numpy(np.asarray(idx, dtype=np.uint32).view(np.int32).copy()).to(dev)
            out = torch.full((len(lens) * 65 + 64,), 0xCD, dtype=torch.uint8, device=dev)
            stream.synchronize()
            ps.multi_scalar_mult_segments_device(n, dk.data_ptr(), di.data_ptr(), off, out.data_ptr(), stream.cuda_stream)
            got = out.cpu().numpy()
        assert np.array_equal(got[:len(lens) * 65].reshape(-1, 65), host)
        assert (got[len(lens) * 65:] == 0xCD).all()                        # nothing written behind the records
        # dense, resident scalars only
        dlens = [m, 0, m - 1]
        dks = rand_scalars(rnd, sum(dlens))
        with torch.cuda.stream(stream):
            dk = torch.from_numpy(np.frombuffer(b"".join(dks), dtype=np.uint8).copy()).to(dev)
            out = torch.zeros(len(dlens) * 65, dtype=torch.uint8, device=dev)
            stream.synchronize()
            ps.multi_scalar_mult_segments_device(sum(dlens), dk.data_ptr(), None, offsets_of(dlens), out.data_ptr(), stream.cuda_stream)
            got = out.cpu().numpy().reshape(-1, 65)
        assert [bytes(r) for r in got] == expect_segments(oracle, dks, dense_points(members, dlens), dlens)
    finally:
        ps.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(eng, pool, sets, monkeypatch):
    import secp256k1_voi_amd as S
    lib = eng._lib
    pts = pool[1]
    rnd = random.Random(8)

    def create_rc(records, c):
        arr = np.frombuffer(b"".join(records), dtype=np.uint8).copy()
        out = C.c_void_p(0x1234)
        rc = lib.s2k_pointset_create(eng._h, len(records), arr.ctypes.data, c, C.byref(out))
        if rc == 0:
            lib.s2k_pointset_destroy(out)
        else:
            assert not out.value                          # no set is made
        return rc
    off_curve = bytearray(pts[1]); off_curve[64] ^= 1
    x0 = next(x for x in range(1, 1000) if R.lift_x(x, False) is not None)
    gx, gy = R.lift_x(x0, False)
    assert create_rc([b"\x04" + b32(gx) + b32(gy)], 4) == 0                             # (the canonical form of that point is fine)
    non_canonical = b"\x04" + b32(R.P + x0) + b32(gy)
    for c in WIDTHS:
        for bad in (bytes(off_curve), non_canonical, b"\x02" + pts[1][1:], b"\x01" + bytes(64)):
            assert create_rc([pts[0], bad, pts[2]], c) == ERR_ARG
            with pytest.raises(S.EngineError):
                eng.pointset_create([pts[0], bad], c)
    assert create_rc(pts[:2], 5) == ERR_ARG and create_rc(pts[:2], 16) == ERR_ARG and create_rc(pts[:2], -1) == ERR_ARG
    out = C.c_void_p()
    assert lib.s2k_pointset_create(eng._h, 0, None, 4, C.byref(out)) == ERR_ARG
    assert lib.s2k_pointset_create(eng._h, 2, None, 4, C.byref(out)) == ERR_ARG
    arr = np.frombuffer(b"".join(pts[:2]), dtype=np.uint8).copy()
    assert lib.s2k_pointset_create(eng._h, 2, arr.ctypes.data, 4, None) == ERR_ARG
    for c in WIDTHS:
        ps = sets(c, 16)
        ks = rand_scalars(rnd, 40)
        idx = [rnd.randrange(16) for _ in range(40)]
        good = ps.multi_scalar_mult_segments(ks, [0, 10, 40], idx)
        for at, v in ((0, 16), (39, 16), (17, 0xFFFFFFFF)):                             # an index that names no point
            bad = list(idx); bad[at] = v
            with pytest.raises(S.EngineError, match="-3"):
                ps.multi_scalar_mult_segments(ks, [0, 10, 40], bad)
            monkeypatch.setenv("S2K_POINTSET_CROSSOVER", "16")                          # ... also on the gathered route
            with pytest.raises(S.EngineError, match="-3"):
                ps.multi_scalar_mult_segments(ks, [0, 10, 40], bad)
            monkeypatch.delenv("S2K_POINTSET_CROSSOVER")
        assert np.array_equal(ps.multi_scalar_mult_segments(ks, [0, 10, 40], idx), good)   # (the set is as good as before)
        for off in ([1, 40], [0, 30, 20, 40], [0, 39], [0, 41], []):
            with pytest.raises(ValueError):
                ps.multi_scalar_mult_segments(ks, off, idx)
        with pytest.raises(ValueError):
            ps.multi_scalar_mult_segments(ks, [0, 40], idx[:39])
        # through the C-ABI itself: S2K_ERR_ARG, nothing written
        kk, ii = np.frombuffer(b"".join(ks), np.uint8).copy(), np.asarray(idx, dtype=np.uint32)
        rec = np.full(3 * 65, 0xAB, dtype=np.uint8)
        call = lib.s2k_pointset_multi_scalar_mult_segments
        for off in ([1, 10, 40], [0, 30, 20, 40], [0, 10, 39], [0, 10, 41]):
            o = np.asarray(off, dtype=np.uint64)
            assert call(eng._h, ps._k, 40, kk.ctypes.data, ii.ctypes.data, 2, o.ctypes.data, rec.ctypes.data) == ERR_ARG
        o = np.asarray([0, 17, 40], dtype=np.uint64)
        assert call(eng._h, ps._k, 40, kk.ctypes.data, None, 2, o.ctypes.data, rec.ctypes.data) == ERR_ARG      # dense: 17 and 23 terms, 16 points
        assert call(eng._h, ps._k, 40, None, ii.ctypes.data, 2, o.ctypes.data, rec.ctypes.data) == ERR_ARG
        assert call(eng._h, ps._k, 40, kk.ctypes.data, ii.ctypes.data, 2, None, rec.ctypes.data) == ERR_ARG
        assert call(eng._h, ps._k, 40, kk.ctypes.data, ii.ctypes.data, 2, o.ctypes.data, None) == ERR_ARG
        assert call(eng._h, None, 40, kk.ctypes.data, ii.ctypes.data, 2, o.ctypes.data, rec.ctypes.data) == ERR_ARG
        assert (rec == 0xAB).all()
    # a set used with another context
    other = S.Engine(0)
    try:
        ps = sets(4, 16)
        with pytest.raises(S.EngineError, match="-3"):
            other._check(lib.s2k_pointset_multi_scalar_mult_segments(other._h, ps._k, 0, None, None, 1, np.zeros(2, np.uint64).ctypes.data,
                                                                     np.zeros(65, np.uint8).ctypes.data))
    finally:
        other.close()
    # automatic width: 8 bits on an empty device; under a budget 4, and below that S2K_ERR_NOMEM
    b8, b4 = 16 * S.pointset_geometry(8)[2], 16 * S.pointset_geometry(4)[2]
    auto = eng.pointset_create(pts[:16], 0)
    assert auto.window_bits() == 8 and auto.device_bytes() >= b8
    auto.close()
    try:
        lib.s2k_set_table_memory_budgets(b8, 0)            # 8 bits would take all of it, not half
        auto = eng.pointset_create(pts[:16], 0)
        assert auto.window_bits() == 4 and b4 <= auto.device_bytes() < b8
        ks = rand_scalars(rnd, 16)
        assert np.array_equal(auto.multi_scalar_mult_segments(ks, [0, 16]), sets(8, 16).multi_scalar_mult_segments(ks, [0, 16]))
        auto.close()
        assert create_rc(pts[:16], 8) == 0                 # an explicit width only has to fit
        lib.s2k_set_table_memory_budgets(b4, 0)
        assert create_rc(pts[:16], 0) == ERR_NOMEM and create_rc(pts[:16], 8) == ERR_NOMEM and create_rc(pts[:16], 4) == 0
        lib.s2k_set_table_memory_budgets(b4 - 1, 0)
        assert create_rc(pts[:16], 4) == ERR_NOMEM
    finally:
        lib.s2k_set_table_memory_budgets(0, 0)


# ---- 9. two sets of one context ----------------------------------------------------------------------------------------------
def test_two_sets_alternately(eng, oracle, pool):
    rnd = random.Random(9)
    pts = pool[1]
    a, b = eng.pointset_create(pts[:10], 8), eng.pointset_create(pts[10:30], 4)
    try:
        lens = [10, 0, 3, 10]
        ks = rand_scalars(rnd, sum(lens))
        ea = expect_segments(oracle, ks, dense_points(pts[:10], lens), lens)
        eb = expect_segments(oracle, ks, dense_points(pts[10:30], lens), lens)
        for _ in range(3):
            assert run(a, ks, lens) == ea
            assert run(b, ks, lens) == eb
        a.close()
        assert run(b, ks, lens) == eb
        c = eng.pointset_create(pts[5:9], 8)              # (may well reuse the memory of the set just destroyed)
        assert run(b, ks, lens) == eb
        assert run(c, ks[:4], [4]) == expect_segments(oracle, ks[:4], pts[5:9], [4])
        c.close()
    finally:
        a.close()
        b.close()
