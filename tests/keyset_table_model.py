"""What every table entry of a key set is: a scalar multiple m * Q of the key Q, m known mod n, and the bytes it is stored
as (KeySet.debug_entries / s2k_debug_keyset_entries read them back).  Pure Python, no device.

The endomorphism phi(x, y) = (beta x, y) acts as lambda (tests/pyref.py).  For the affine (x, y) of m * Q the tables hold
(W^2 x, W^3 y) and, in the base tables, beta W^2 x, with W the one Z all entries of a key share: the model prescribes no W,
it takes the one the set gives.  The lead pair of a base table has no beta column - no ladder reads the endomorphism of a
starting point - and its 32 bytes are zero.

Sections (the order of the entries in each is the order of the tables):
  base, window layouts (CHUNKS, JOINT, JOINT5, JOINT6)   entry 8 c + a = (2 a + 1) 16^c Q, c < 32, a < 8; then L + phi(L),
                                                         L - phi(L), L = 2^128 Q
  base, COMB                                             E[idx] = B_6 + sum_{t<6} (2 idx_t - 1) B_t, B_t = 2^(19 t) Q
                                                         (test_comb_model.entry_scalar); then the pair of L = 2^115 Q
  joint, W-bit digits (JOINT: W = 4, 32 positions)       entry i PER_POS + 2 (a NE + b) + s = (2 a + 1) B_i +
                                                         (-1)^s phi((2 b + 1) B_i), B_i = 2^(W i) Q; W = 5, 6: then the pair
                                                         of 2^(W POS) Q

The points come from affine additions with one shared inversion per batch (Montgomery's trick), so that the 45 058 entries
of a JOINT6 key cost well under a second; tests/test_keyset_table_model.py holds every definition against the oracle's scalar
multiplication."""
import numpy as np

import pyref as R
from test_comb_model import LEAD_LOG2 as COMB_LEAD_LOG2, SPACING as COMB_SPACING, entry_scalar as comb_entry_scalar
from test_coz_model import BETA

P, N, LAMBDA = R.P, R.N, R.LAMBDA
CHUNKS, JOINT, JOINT5, JOINT6, COMB = 1, 2, 3, 4, 5        # S2K_KEYSET_*
LAYOUTS = (CHUNKS, JOINT, JOINT5, JOINT6, COMB)
WIDTH = {JOINT: 4, JOINT5: 5, JOINT6: 6}                    # digit width of the joint tables
WINDOW_LEAD_LOG2 = 128


class Geom:
    """the numbers of kjw_geom<W> (W = 4: the 32 x 128 entries of KJ_*, which end without a lead pair)"""

    def __init__(self, w):
        self.W, self.NE, self.POS = w, 1 << (w - 1), (128 + w - 1) // w
        self.PER_POS = 2 * self.NE * self.NE
        self.LEAD = self.POS * self.PER_POS
        self.ENTRIES = self.LEAD + (2 if w > 4 else 0)
        self.ENTRY_BYTES = 80 if w == 4 else 64


def joint_geom(layout):
    return Geom(WIDTH[layout])


def base_entries(layout):
    return 66 if layout == COMB else 258


def joint_entries(layout):
    return joint_geom(layout).ENTRIES if layout in WIDTH else 0


def table_bytes_per_key(layout):
    """what s2k_keyset_geometry reports: the slots of the base table (entries and build scratch, 128 bytes each) and the joint table"""
    if layout == COMB:
        return 80 * 128
    g = joint_geom(layout) if layout in WIDTH else None
    return 288 * 128 + (g.ENTRIES * g.ENTRY_BYTES if g else 0)


def additions_per_signature(layout):
    return {CHUNKS: 64, COMB: 2 * COMB_SPACING}.get(layout) or joint_geom(layout).POS


# ==== scalars: entry -> m mod n =============================================================================================
def _pair(m):
    return [m * (1 + LAMBDA) % N, m * (1 - LAMBDA) % N]


def base_scalar(layout, idx):
    if layout == COMB:
        return comb_entry_scalar(idx) % N if idx < 64 else _pair(1 << COMB_LEAD_LOG2)[idx - 64]
    return (2 * (idx % 8) + 1) << (4 * (idx // 8)) if idx < 256 else _pair(1 << WINDOW_LEAD_LOG2)[idx - 256]


def joint_scalar(layout, idx):
    g = joint_geom(layout)
    if idx >= g.LEAD:
        assert g.W > 4 and idx < g.LEAD + 2
        return _pair(1 << (g.W * g.POS))[idx - g.LEAD]
    i, k = divmod(idx, g.PER_POS)
    a, b, s = k // 2 // g.NE, k // 2 % g.NE, k & 1
    return (((2 * a + 1) + (-1) ** s * LAMBDA * (2 * b + 1)) << (g.W * i)) % N


# ==== points ================================================================================================================
def _inv_all(v):
    """the inverses of a list of non-zero residues, one inversion for all"""
    pre, acc = [], 1
    for x in v:
        pre.append(acc)
        acc = acc * x % P
    inv = pow(acc, -1, P)
    out = [0] * len(v)
    for i in range(len(v) - 1, -1, -1):
        out[i] = inv * pre[i] % P
        inv = inv * v[i] % P
    return out


def _add_all(pairs):
    """p + q for every pair of affine points with different x"""
    out = []
    for ((x1, y1), (x2, y2)), di in zip(pairs, _inv_all([(q[0] - p[0]) % P for p, q in pairs])):
        lam = (y2 - y1) * di % P
        x3 = (lam * lam - x1 - x2) % P
        out.append((x3, (lam * (x1 - x3) - y1) % P))
    return out


def _double(pt):
    x, y = pt
    lam = 3 * x * x * pow(2 * y, -1, P) % P
    x3 = (lam * lam - 2 * x) % P
    return (x3, (lam * (x - x3) - y) % P)


def phi(pt):
    return (pt[0] * BETA % P, pt[1])


def neg(pt):
    return (pt[0], (P - pt[1]) % P)


class KeyTables:
    """the table entries of one key Q = (x, y) as affine points; every section on demand, the doublings 2^k Q kept"""

    def __init__(self, Q):
        self.Q = Q
        self._pow = [Q]

    def pow2(self, k):
        while len(self._pow) <= k:
            self._pow.append(_double(self._pow[-1]))
        return self._pow[k]

    def _lead_pair(self, log2):
        L = self.pow2(log2)
        return _add_all([(L, phi(L)), (L, neg(phi(L)))])

    def odd_multiples(self, bases, ne):
        """[(2 a + 1) B for a < ne] for every B of `bases`"""
        twice = [_double(b) for b in bases]
        cur, out = list(bases), [[b] for b in bases]
        for _ in range(1, ne):
            cur = _add_all(list(zip(cur, twice)))
            for o, c in zip(out, cur):
                o.append(c)
        return out

    def base(self, layout):
        """section 1, in the order of the table"""
        if layout == COMB:
            pts = [self.pow2(COMB_SPACING * 6)]              # the signs of the teeth t = 5 .. 0 taken one by one: idx_t = 1 is +
            for t in range(5, -1, -1):
                b = self.pow2(COMB_SPACING * t)
                minus, plus = _add_all([(p, neg(b)) for p in pts]), _add_all([(p, b) for p in pts])
                pts = [q for pair in zip(minus, plus) for q in pair]
            # pts is ordered by (idx_5, idx_4, .., idx_0), the most significant tooth first: that is idx itself
            return pts + self._lead_pair(COMB_LEAD_LOG2)
        chunks = self.odd_multiples([self.pow2(4 * c) for c in range(32)], 8)
        return [p for ch in chunks for p in ch] + self._lead_pair(WINDOW_LEAD_LOG2)

    def joint_positions(self, layout, positions):
        """{i: the PER_POS entries of position i} of section 2"""
        g = joint_geom(layout)
        odd = self.odd_multiples([self.pow2(g.W * i) for i in positions], g.NE)
        out = {}
        for i, e in zip(positions, odd):
            images = [phi(p) for p in e]
            plus = _add_all([(ea, pb) for ea in e for pb in images])
            minus = _add_all([(ea, neg(pb)) for ea in e for pb in images])
            out[i] = [q for pair in zip(plus, minus) for q in pair]
        return out

    def joint_lead(self, layout):
        g = joint_geom(layout)
        assert g.W > 4
        return self._lead_pair(g.W * g.POS)

    def joint(self, layout):
        """all of section 2"""
        g = joint_geom(layout)
        per = self.joint_positions(layout, list(range(g.POS)))
        return [p for i in range(g.POS) for p in per[i]] + (self.joint_lead(layout) if g.W > 4 else [])


# ==== stored bytes ==========================================================================================================
def stored(points, w, beta_column=False, lead=0):
    """the (len(points), 64 or 96) uint8 array of (W^2 x, W^3 y[, beta W^2 x]); the last `lead` rows with a zero beta column"""
    assert 0 < w < P
    w2 = w * w % P
    w3 = w2 * w % P
    rows = []
    for k, (x, y) in enumerate(points):
        sx = x * w2 % P
        row = sx.to_bytes(32, "big") + (y * w3 % P).to_bytes(32, "big")
        if beta_column:
            row += bytes(32) if k >= len(points) - lead else (sx * BETA % P).to_bytes(32, "big")
        rows.append(row)
    return np.frombuffer(b"".join(rows), np.uint8).reshape(len(points), 96 if beta_column else 64)


def stored_base(points, w):
    return stored(points, w, beta_column=True, lead=2)
