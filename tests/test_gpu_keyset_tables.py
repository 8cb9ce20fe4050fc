"""The tables of a key set read back entry by entry (KeySet.debug_entries / s2k_debug_keyset_entries) and compared, byte for
byte, with tests/keyset_table_model.py: every entry is the scalar multiple m * Q the model says, stored as (W^2 x, W^3 y[,
beta W^2 x]) under the W the set reports for the key.  Nothing is tolerated.

What is read: sets created whole in every layout at 1, 5 and 33 keys (33 x 26 and 33 x 22 lanes of the wide build kernels end
in a partial 64-lane block, and keys straddle block borders), rows an append built (first > 0, validity bytes at unaligned
addresses), sets moved by reserve(), and rows replace() / remove() scattered from a staging set in several pieces.

Keys: the private scalars 1, 2, n - 1, lambda, (n - 1) / 2 and seeded random ones; between them rows that are no key - off the
curve, a coordinate >= p, 64 zero bytes - of which only valid_keys() is asserted (their rows are unspecified), while their
valid neighbours' rows must be exact.  At 33 keys the keys 0 (d = 1), 2 (d = lambda) and 32 are compared in full and every other valid key in
section 0, all of section 1 and, in section 2, the first and the last position and the lead pair: they are left out of the full
comparison only to keep the Python model's time down.

A failure names the key, the section and the entry (with its position, a, b and sign)."""
import numpy as np
import pytest

import keyset_table_model as M
import pyref as R

pytestmark = pytest.mark.gpu
P, N = R.P, R.N
ERR_ARG = -3
LAYOUT_NAMES = {M.CHUNKS: "CHUNKS", M.JOINT: "JOINT", M.JOINT5: "JOINT5", M.JOINT6: "JOINT6", M.COMB: "COMB"}
SPECIAL = [1, 2, N - 1, R.LAMBDA, (N - 1) // 2]
NRANDOM = 110
ZERO = bytes(64)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    S.debug_keyset_replace_piece(0)
    e.close()


class Universe:
    """the valid keys (points and bytes), and the model of each, computed once per module: the base table, the whole joint
    table and its checked part, per (key, layout)"""

    def __init__(self):
        rng = np.random.default_rng(3301)
        scalars = SPECIAL + [int.from_bytes(rng.bytes(32), "big") % (N - 1) + 1 for _ in range(NRANDOM)]
        self.points = [R.mul(d, R.G) for d in scalars]
        self.bytes = [R.b32(x) + R.b32(y) for x, y in self.points]
        self.by_bytes = dict(zip(self.bytes, self.points))
        self._tables, self._memo = {}, {}

    def tables(self, Q):
        if Q not in self._tables:
            self._tables[Q] = M.KeyTables(Q)
        return self._tables[Q]

    def _get(self, what, Q, layout, make):
        key = (what, Q, layout if what != "base" or layout == M.COMB else M.CHUNKS)      # (one base table for the four window layouts)
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def base(self, Q, layout):
        return self._get("base", Q, layout, lambda: self.tables(Q).base(layout))

    def joint(self, Q, layout):
        return self._get("joint", Q, layout, lambda: self.tables(Q).joint(layout))

    def joint_ends(self, Q, layout):
        """position 0, position POS - 1 (chunks 0 and 31 of JOINT), and the lead pair of the wide layouts"""
        def make():
            g = M.joint_geom(layout)
            per = self.tables(Q).joint_positions(layout, [0, g.POS - 1])
            return per[0], per[g.POS - 1], (self.tables(Q).joint_lead(layout) if g.W > 4 else [])
        return self._get("ends", Q, layout, make)

    def off_curve(self, i):
        x, y = self.points[i]
        return R.b32(x) + R.b32((y + 1) % P)

    def big(self, i):
        """X >= p: x + p still fits 32 bytes for a small x - here the coordinate is p + 5, whatever the Y"""
        return R.b32(P + 5) + R.b32(self.points[i][1])


@pytest.fixture(scope="module")
def uni():
    return Universe()


def _arr(rows):
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, 64)


INVALID33 = {1: "off", 6: "zero", 9: "big", 16: "big", 20: "off", 31: "zero"}


def _rows33(uni):
    """33 rows: 27 keys - d = 1 at row 0, lambda at row 2, then 2, n - 1, (n - 1) / 2 and random ones - and between them, never
    in place of one, the three kinds of rows that are no key (one beside the last key); rows 0, 2 and 32 are keys"""
    one, two, minus_one, lam, half = uni.bytes[:5]
    v = iter([one, lam, two, minus_one, half] + uni.bytes[5:])
    bad = {"off": uni.off_curve, "big": uni.big, "zero": lambda i: ZERO}
    rows = [bad[INVALID33[k]](40 + k) if k in INVALID33 else next(v) for k in range(33)]
    assert [k for k, r in enumerate(rows) if r in uni.bytes[:5]] == [0, 2, 3, 4, 5]        # every special key is in the set
    return rows


def _rows(uni, n):
    """the key lists of the created sets: the same keys at the checked rows of every size, so that the model of a key is
    computed once.  Five rows: d = 1, X >= p, lambda, 64 zero bytes, the last key of the 33"""
    r = _rows33(uni)
    if n == 33:
        return r
    if n == 5:
        return [r[0], r[9], r[2], r[6], r[32]]
    assert n == 1
    return [r[0]]


def _describe(layout, section, idx):
    if section == 1:
        if layout == M.COMB:
            return "comb entry idx=%d" % idx if idx < 64 else "lead pair %d" % (idx - 64)
        return "chunk %d, a=%d" % (idx // 8, idx % 8) if idx < 256 else "lead pair %d" % (idx - 256)
    g = M.joint_geom(layout)
    if idx >= g.LEAD:
        return "lead pair %d" % (idx - g.LEAD)
    i, k = divmod(idx, g.PER_POS)
    return "position %d, a=%d, b=%d, s=%d" % (i, k // 2 // g.NE, k // 2 % g.NE, k & 1)


def _same(got, exp, layout, key, section, first, note):
    assert got.shape == exp.shape, (note, key, section, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).any(axis=1))
    if bad.size:
        lines = ["%s layout %s: key %d, section %d, entry %d (%s)" % (note, LAYOUT_NAMES[layout], key, section, first + int(b),
                                                                    _describe(layout, section, first + int(b))) for b in bad[:8]]
        b = int(bad[0])
        pytest.fail("%d wrong entries\n%s\n got %s\n want %s" % (bad.size, "\n".join(lines), bytes(got[b]).hex(), bytes(exp[b]).hex()))


def _below_p(got, layout, key, first, note):
    """every stored word string of a wide entry is a canonical value"""
    vals = got.reshape(-1, 32)
    # p = 2^256 - 2^32 - 977: a 32-byte string is >= p only if its first 27 bytes are all ones
    for r in np.flatnonzero((vals[:, :27] == 0xFF).all(axis=1)):
        assert int.from_bytes(bytes(vals[r]), "big") < P, "%s layout %s: key %d, section 2, entry %d (%s): a coordinate >= p" % (
            note, LAYOUT_NAMES[layout], key, first + r // 2, _describe(layout, 2, first + r // 2))


def check_key(ks, uni, key, key_bytes, full, note=""):
    """the tables of row `key`, which holds the valid key `key_bytes`, against the model"""
    layout = ks.layout()
    Q = uni.by_bytes[bytes(key_bytes)]
    w = int.from_bytes(bytes(ks.debug_entries(key, 0)[0]), "big")
    assert 0 < w < P, (note, key, w)
    _same(ks.debug_entries(key, 1), M.stored_base(uni.base(Q, layout), w), layout, key, 1, 0, note)
    if layout not in M.WIDTH:
        return
    g = M.joint_geom(layout)
    if full:
        parts = [(0, uni.joint(Q, layout))]
    else:
        first, last, lead = uni.joint_ends(Q, layout)
        parts = [(0, first), (g.LEAD - g.PER_POS, last)] + ([(g.LEAD, lead)] if lead else [])
    for start, pts in parts:
        got = ks.debug_entries(key, 2, start, len(pts))
        if g.W > 4:
            _below_p(got, layout, key, start, note)
        _same(got, M.stored(pts, w), layout, key, 2, start, note)


def check_set(ks, uni, rows, full_keys, note="", only=None):
    """valid_keys() of the whole set; every valid row (or the rows `only`) against the model, those of full_keys in full"""
    valid = [bytes(r) in uni.by_bytes for r in rows]
    assert len(ks) == len(rows) and list(ks.valid_keys()) == [int(v) for v in valid], note
    checked = 0
    for k in (range(len(rows)) if only is None else only):
        if valid[k]:
            check_key(ks, uni, k, rows[k], k in full_keys, note)
            checked += 1
    return checked


LAYOUTS = [M.CHUNKS, M.JOINT, M.JOINT5, M.JOINT6, M.COMB]


@pytest.mark.parametrize("n", [1, 5, 33])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[LAYOUT_NAMES[l] for l in LAYOUTS])
def test_created_set(eng, uni, layout, n):
    rows = _rows(uni, n)
    full = {0, 2, n - 1} if n > 1 else {0}
    assert all(bytes(rows[k]) in uni.by_bytes for k in full) and len(full) == min(n, 3)
    ks = eng.keyset_create(_arr(rows), layout)
    try:
        assert ks.layout() == layout
        if n == 33:     # the keys of the private scalars 1, 2, n - 1, lambda, (n - 1) / 2 are all among the valid rows
            assert all(k in rows and k in uni.by_bytes for k in uni.bytes[:len(SPECIAL)]) and uni.points[1] == R.mul(2, R.G)
        checked = check_set(ks, uni, rows, full, "created with %d keys," % n)
        assert checked == sum(bytes(r) in uni.by_bytes for r in rows) == {1: 1, 5: 3, 33: 27}[n]      # no valid key is skipped
    finally:
        ks.close()


@pytest.mark.parametrize("layout", [M.JOINT5, M.COMB, M.CHUNKS], ids=["JOINT5", "COMB", "CHUNKS"])
def test_appended_rows(eng, uni, layout):
    """appends of 1, 7 and 64 keys behind 5: first = 5, 6, 13 - rows and validity bytes at unaligned addresses, and at 64 keys
    more than one block of the build kernels.  Bad rows sit inside the 7 and the 64"""
    rows = _rows(uni, 5)
    ks = eng.keyset_create(_arr(rows), layout, capacity=80)
    try:
        fresh = iter(uni.bytes[40:])
        for count in (1, 7, 64):
            new = [next(fresh) for _ in range(count)]
            if count > 1:
                new[1] = uni.off_curve(50)
                new[count - 2] = ZERO
            if count == 64:
                new[30] = uni.big(51)
            before = len(rows)
            assert ks.append(_arr(new)) == before
            rows = rows + new
            note = "after the append of %d keys at %d," % (count, before)
            assert check_set(ks, uni, rows, set(range(len(rows))), note, only=sorted({before - 1, before, before + count - 1})) == min(3, count + 1)
        # and nothing the appends passed over has moved: every valid row once more, the earlier ones at their ends
        check_set(ks, uni, rows, {0, 2, 4}, "after all appends,")
    finally:
        ks.close()


@pytest.mark.parametrize("layout", [M.JOINT5, M.JOINT6, M.COMB], ids=["JOINT5", "JOINT6", "COMB"])
def test_reserved_set(eng, uni, layout):
    """reserve() copies every section to buffers laid out for another capacity; an append then builds behind the copied rows"""
    rows = _rows(uni, 5)
    full = {0, 2, 4}
    ks = eng.keyset_create(_arr(rows), layout)
    try:
        check_set(ks, uni, rows, full, "before reserve,")
        ks.reserve(12)
        assert ks.capacity() == 12
        check_set(ks, uni, rows, full, "after reserve(12),")
        new = [uni.bytes[60], uni.off_curve(61), uni.bytes[62]]
        assert ks.append(_arr(new)) == 5
        rows = rows + new
        check_set(ks, uni, rows, full | {5, 7}, "after reserve(12) and an append of 3,")
    finally:
        ks.close()


@pytest.mark.parametrize("layout", [M.JOINT5, M.JOINT, M.COMB], ids=["JOINT5", "JOINT", "COMB"])
def test_replaced_and_removed_rows(eng, uni, layout):
    """14 rows; seven slots - the first, the last, scattered ones, given out of order - replaced in pieces of three (three
    pieces, the last of one), one of the new rows 64 zero bytes, then a row removed: the replaced rows are the new keys', the
    removed ones read invalid, and every row beside a replaced slot is what it was"""
    import secp256k1_voi_amd as S
    rows = list(uni.bytes[5:19])
    rows[4] = uni.off_curve(70)
    ks = eng.keyset_create(_arr(rows), layout)
    everything = set(range(14))
    try:
        check_set(ks, uni, rows, {0, 13}, "before replace,")
        S.debug_keyset_replace_piece(3)
        slots = [13, 0, 5, 8, 3, 10, 6]
        new = [uni.bytes[80 + i] for i in range(7)]
        new[6] = ZERO
        ks.replace(slots, _arr(new))
        for s, k in zip(slots, new):
            rows[s] = k
        ks.remove([11])
        rows[11] = ZERO
        S.debug_keyset_replace_piece(0)
        valid = ks.valid_keys()
        assert valid[6] == 0 and valid[11] == 0 and valid[4] == 0
        checked = check_set(ks, uni, rows, everything, "after replace and remove,")
        assert checked == 11                                  # 14 rows less the off-curve one and the two removed
    finally:
        S.debug_keyset_replace_piece(0)
        ks.close()


def test_refusals(eng, uni):
    """S2K_ERR_ARG with the output untouched; a good call right afterwards"""
    import secp256k1_voi_amd as S
    lib = S.load_library()
    rows = _rows(uni, 5)
    for layout in (M.JOINT5, M.JOINT, M.CHUNKS, M.COMB):
        ks = eng.keyset_create(_arr(rows), layout, capacity=9)
        try:
            n1, n2 = M.base_entries(layout), M.joint_entries(layout)
            buf = np.full(4 * 96, 0xA5, np.uint8)
            bad = [(ks._k, 0, 0, 0, 1, None), (None, 0, 0, 0, 1, buf.ctypes.data),
                   (ks._k, 5, 1, 0, 1, buf.ctypes.data), (ks._k, 8, 0, 0, 1, buf.ctypes.data), (ks._k, 2**40, 1, 0, 1, buf.ctypes.data),
                   (ks._k, 0, 3, 0, 1, buf.ctypes.data), (ks._k, 0, -1, 0, 1, buf.ctypes.data),
                   (ks._k, 0, 1, n1, 1, buf.ctypes.data), (ks._k, 0, 1, n1 - 1, 2, buf.ctypes.data), (ks._k, 0, 1, 0, n1 + 1, buf.ctypes.data),
                   (ks._k, 0, 1, 2**63, 2**63, buf.ctypes.data), (ks._k, 0, 1, 2, 2**64 - 1, buf.ctypes.data),
                   (ks._k, 0, 0, 0, 0, buf.ctypes.data), (ks._k, 0, 0, 0, 2, buf.ctypes.data), (ks._k, 0, 0, 1, 1, buf.ctypes.data)]
            if n2:
                bad += [(ks._k, 0, 2, n2, 1, buf.ctypes.data), (ks._k, 0, 2, n2 - 1, 2, buf.ctypes.data), (ks._k, 0, 2, 0, n2 + 1, buf.ctypes.data)]
            else:
                bad += [(ks._k, 0, 2, 0, 1, buf.ctypes.data), (ks._k, 0, 2, 0, 0, buf.ctypes.data)]
            for args in bad:
                assert lib.s2k_debug_keyset_entries(*args) == ERR_ARG, (layout, args[1:5])
                assert (buf == 0xA5).all(), (layout, args[1:5])
            # count == 0 is no error and writes nothing, at either end of a section
            for section, total in ((1, n1), (2, n2)) if n2 else ((1, n1),):
                assert lib.s2k_debug_keyset_entries(ks._k, 0, section, 0, 0, buf.ctypes.data) == 0
                assert lib.s2k_debug_keyset_entries(ks._k, 0, section, total, 0, buf.ctypes.data) == 0
            assert (buf == 0xA5).all()
            # a good call right afterwards: the last two entries of section 1 through the raw call are what the method gives
            assert lib.s2k_debug_keyset_entries(ks._k, 4, 1, n1 - 2, 2, buf.ctypes.data) == 0
            assert np.array_equal(buf[:192].reshape(2, 96), ks.debug_entries(4, 1)[-2:]) and (buf[192:] == 0xA5).all()
            check_key(ks, uni, 4, rows[4], True, "after the refusals,")
            with pytest.raises(S.EngineError):
                ks.debug_entries(5, 1)
            # the sections' sizes are the library's, and the method leaves the refusing to it
            import ctypes
            size = ctypes.c_size_t(77)
            for section, total in ((0, 1), (1, n1), (2, n2)):
                rc = lib.s2k_debug_keyset_section_entries(ks._k, section, ctypes.byref(size))
                assert (rc, size.value) == ((0, total) if total else (ERR_ARG, 77)), (layout, section)
                size.value = 77
            for args in ((ks._k, 3, ctypes.byref(size)), (ks._k, -1, ctypes.byref(size)), (None, 1, ctypes.byref(size)), (ks._k, 1, None)):
                assert lib.s2k_debug_keyset_section_entries(*args) == ERR_ARG and size.value == 77
            assert ks.debug_entries(0, 1, n1 - 1).shape == (1, 96) and ks.debug_entries(0, 1, n1).shape == (0, 96)
            for section, first in ((1, n1 + 1), (0, 1), (3, 0)) + (() if n2 else ((2, 0),)):
                with pytest.raises(S.EngineError):
                    ks.debug_entries(0, section, first)
        finally:
            ks.close()
