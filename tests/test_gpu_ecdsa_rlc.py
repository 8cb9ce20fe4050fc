"""Whole-batch verification of recoverable ECDSA signatures on the device (s2k_ecdsa_batch_verify_rlc,
s2k_ecdsa_verify_recoverable_batch_bisect).  Every expected verdict is oracle.ecdsa_recover(digest, r, s, v) compared with
the supplied key (and s <= n/2 under the flag), never something the engine computed.  Large batches are a small
oracle-checked batch tiled with numpy: a verdict is a function of the item alone, and the coefficients differ per index.
"""
import ctypes as C
import random

import numpy as np
import pytest

import ecdsa_rlc_model as M
import pyref
from pyref import N, P, b32

pytestmark = pytest.mark.gpu

PREP_M = 6
SEED = bytes(range(32))
ERR_ARG = -3


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    return S.Engine(0)


@pytest.fixture(scope="module")
def base_mult(oracle):
    return lambda k: pyref.dec65(oracle.scalar_base_mult_vartime(b32(k)))


def truth(oracle, b, idx=None, reject=False):
    """the contract's verdict of the items idx (all of them by default), from the oracle"""
    idx = range(len(b["v"])) if idx is None else idx
    out = np.zeros(len(idx), np.uint8)
    for k, i in enumerate(idx):
        rec = oracle.ecdsa_recover(bytes(b["digest"][i]), bytes(b["r"][i]), bytes(b["s"][i]), int(b["v"][i]))
        good = rec is not None and rec == b"\x04" + bytes(b["pub"][i])
        if good and reject:
            good = not oracle.fn_is_gt_half_n(bytes(b["s"][i]))
        out[k] = good
    return out


def args(b):
    return b["pub"], b["digest"], b["r"], b["s"], b["v"]


def copy(b):
    return {k: v.copy() for k, v in b.items()}


def tiled(b, n):
    return {k: np.resize(v, (n,) + v.shape[1:]) for k, v in b.items()}


def high_x_item(oracle, seed):
    dg, r, s = M.high_x_tuple(seed)
    return pyref.dec65(oracle.ecdsa_recover(dg, b32(r), b32(s), 3)), dg, r, s, 3


def check_both(eng, b, expect, reject=False):
    """the whole-batch call says whether all are good; the bisect call gives the expected verdicts"""
    for seed in (SEED, None):
        assert eng.ecdsa_batch_verify_rlc(*args(b), seed32=seed, reject_malleable=reject) == bool(expect.all())
    got = eng.ecdsa_verify_recoverable_batch(*args(b), seed32=SEED, reject_malleable=reject)
    assert np.array_equal(got, expect), np.nonzero(got != expect)[0][:10]


@pytest.fixture(scope="module")
def good512(oracle, base_mult):
    """512 good items under 7 keys, low s, checked by the oracle once: what the large batches are tiled from"""
    b = M.make_recoverable_batch(512, 7, seed=0x512, base_mult=base_mult)
    assert truth(oracle, b, reject=True).all()
    return b


# ---- 1. accepts ----
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_accepts_good_batches(eng, oracle, base_mult, n):
    for nkeys in sorted({1, min(7, n), n}):
        items = M.make_recoverable_items(n, nkeys, seed=1000 * n + nkeys, high_s_every=5, base_mult=base_mult)
        if n >= 2:
            items[1] = high_x_item(oracle, n)
        b = M.to_arrays(items)
        assert truth(oracle, b).all()
        if n >= 5:
            assert as_int(b["s"][4]) > N // 2                                       # (high s is present)
        check_both(eng, b, np.ones(n, np.uint8))


def test_accepts_a_key_beyond_one_virtual_group(eng, oracle, base_mult, good512):
    """2500 items of ONE key: more than KG_VGROUP = 1024 members, three virtual groups for one key"""
    one = M.make_recoverable_batch(500, 1, seed=0x2500, base_mult=base_mult)
    assert truth(oracle, one).all()
    b = tiled(one, 2500)
    assert len({bytes(k) for k in b["pub"]}) == 1
    check_both(eng, b, np.ones(2500, np.uint8))
    b["digest"][1777, 31] ^= 1
    expect = np.ones(2500, np.uint8)
    expect[1777] = truth(oracle, b, [1777])[0]
    assert expect[1777] == 0
    check_both(eng, b, expect)


def test_device_forms(eng, oracle, good512):
    import torch
    b = tiled(good512, 257)
    dev = [torch.from_numpy(a).cuda() for a in args(b)]
    valid = torch.full((257,), 7, dtype=torch.uint8, device="cuda")
    ptrs = [t.data_ptr() for t in dev]
    assert eng.ecdsa_batch_verify_rlc_device(257, *ptrs, seed32=SEED) is True
    eng.ecdsa_verify_recoverable_batch_device(257, *ptrs, valid.data_ptr(), seed32=SEED)
    torch.cuda.synchronize()
    assert valid.cpu().numpy().all()
    b["v"][200] ^= 1
    dev[4] = torch.from_numpy(b["v"]).cuda()
    ptrs = [t.data_ptr() for t in dev]
    assert eng.ecdsa_batch_verify_rlc_device(257, *ptrs, seed32=SEED) is False
    eng.ecdsa_verify_recoverable_batch_device(257, *ptrs, valid.data_ptr())
    torch.cuda.synchronize()
    expect = np.ones(257, np.uint8)
    expect[200] = truth(oracle, b, [200])[0]
    assert expect[200] == 0 and np.array_equal(valid.cpu().numpy(), expect)


# ---- 2. each way to be bad ----
def put(arr, i, value):
    arr[i] = np.frombuffer(b32(value), np.uint8)


def as_int(row):
    return int.from_bytes(bytes(row), "big")


DAMAGES = {
    "digest bit": lambda b, i: b["digest"].__setitem__((i, 7), b["digest"][i, 7] ^ 0x10),
    "another valid key": lambda b, i: b["pub"].__setitem__(i, b["pub"][(i + 1) % len(b["v"])].copy()),
    "Y ^= 1": lambda b, i: b["pub"].__setitem__((i, 63), b["pub"][i, 63] ^ 1),
    "X = p": lambda b, i: b["pub"].__setitem__((i, slice(0, 32)), np.frombuffer(b32(P), np.uint8)),
    "v ^ 1": lambda b, i: b["v"].__setitem__(i, b["v"][i] ^ 1),
    "v | 2": lambda b, i: b["v"].__setitem__(i, b["v"][i] | 2),
    "v = 4": lambda b, i: b["v"].__setitem__(i, 4),
    "r = 0": lambda b, i: put(b["r"], i, 0),
    "s = 0": lambda b, i: put(b["s"], i, 0),
    "r = n": lambda b, i: put(b["r"], i, N),
    "s = n": lambda b, i: put(b["s"], i, N),
    "s = n + 1": lambda b, i: put(b["s"], i, N + 1),
}


@pytest.mark.parametrize("what", list(DAMAGES) + ["high s under the flag"])
def test_each_way_to_be_bad(eng, oracle, good512, what):
    n = 300
    for i in (0, 299, 150):
        b = tiled(good512, n)
        reject = what == "high s under the flag"
        if reject:                                      # still good without the flag: (r, n - s, v ^ 1)
            put(b["s"], i, N - as_int(b["s"][i]))
            b["v"][i] ^= 1
            assert truth(oracle, b, [i])[0] == 1
        else:
            DAMAGES[what](b, i)
        expect = np.ones(n, np.uint8)
        expect[i] = truth(oracle, b, [i], reject)[0]
        assert expect[i] == 0, (what, i)
        check_both(eng, b, expect, reject)


# ---- 3. lane-mates of items whose s (or r) has no inverse ----
def prep_lanes(n):                                      # k_scalar_prep's lanes, as tests/test_gpu_scalar.py deals them
    return max((n + PREP_M - 1) // PREP_M, min(n, 1 << 16))


def lane_items(t, T, n):
    return [t + j * T for j in range(PREP_M) if t + j * T < n]


def test_lane_mates(eng, oracle, good512):
    """The whole-batch preparation inverts s per lane; the leaf of the bisect call recovers keys behind k_scalar_prep, whose
    lanes share one inversion (of r there) among the items t, t + T, ...: whole lanes of s = 0 / s = n items, single such
    items among good lane-mates, and the same with r."""
    n = (1 << 16) + (1 << 15) + 1
    T = prep_lanes(n)
    assert T == 1 << 16 and len(lane_items(0, T, n)) == 2
    rng = random.Random(n)
    b = tiled(good512, n)
    whole = list(dict.fromkeys(i for t in (0, T - 1, (n - 1) % T, rng.randrange(T), rng.randrange(T)) for i in lane_items(t, T, n)))
    taken = set(whole)
    single = []
    while len(single) < 40:
        i = rng.randrange(n)
        lane = lane_items(i % T, T, n)
        if len(lane) == 2 and not set(lane) & taken:                   # (the lanes from n - T on hold one item only)
            taken.add(i)
            single.append(i)
    damaged = whole + single
    for k, i in enumerate(damaged):
        put(b["r" if k % 4 >= 2 else "s"], i, (0, N)[k % 2])
    expect = np.ones(n, np.uint8)
    expect[damaged] = truth(oracle, b, damaged)
    assert not expect[damaged].any()
    mates = sorted({m for i in single for m in lane_items(i % T, T, n)} - set(damaged))
    assert len(mates) == len(single) and truth(oracle, b, mates).all()
    check_both(eng, b, expect)


# ---- 4. the cancelling pair ----
@pytest.mark.parametrize("at", [(1, 2), (0, 1)])
def test_cancelling_pair(eng, oracle, base_mult, good512, at):
    p1, p2 = M.cancelling_pair(0xCA + at[0], base_mult)
    pair = M.to_arrays([p1, p2])
    b = tiled(good512, 64)
    for k in b:
        b[k][at[0]], b[k][at[1]] = pair[k][0], pair[k][1]
    expect = truth(oracle, b)
    assert [int(i) for i in np.nonzero(expect == 0)[0]] == list(at)
    check_both(eng, b, expect)


# ---- 5. exceptional points in the sum ----
def test_exceptional_points(eng, oracle, base_mult):
    rng = random.Random(5)
    d = rng.randrange(2, N)
    Q, one = base_mult(d), base_mult(1)
    dg = [rng.randbytes(32) for _ in range(8)]
    rep = (Q, dg[0]) + M.sign_recoverable(d, dg[0], rng.randrange(1, N), base_mult=base_mult)
    tw = (Q, dg[1]) + M.sign_recoverable(d, dg[1], rng.randrange(1, N), base_mult=base_mult)
    twin = (Q, dg[1], tw[2], N - tw[3], tw[4] ^ 1)                                    # R and -R both present
    items = [rep] * 64 + [tw, twin,
                          (Q, dg[2]) + M.sign_recoverable(d, dg[2], 1, base_mult=base_mult),          # R = G
                          (one, dg[3]) + M.sign_recoverable(1, dg[3], rng.randrange(1, N), base_mult=base_mult),   # Q = G
                          (Q, dg[4]) + M.sign_recoverable(d, dg[4], d, base_mult=base_mult),          # R = Q
                          (Q, dg[5]) + M.sign_recoverable(d, dg[5], N - d, base_mult=base_mult)]      # R = -Q
    b = M.to_arrays(items)
    n = len(items)
    assert truth(oracle, b).all()
    check_both(eng, b, np.ones(n, np.uint8))
    for i in (17, 65, 68):
        bad = copy(b)
        bad["digest"][i, 0] ^= 0x80
        expect = truth(oracle, bad)
        assert [int(j) for j in np.nonzero(expect == 0)[0]] == [i]
        check_both(eng, bad, expect)


# ---- 6. bisection beyond a leaf ----
def test_bisection_beyond_a_leaf(eng, oracle, good512):
    """Ranges of up to 2^17 items are leaves.  n = 2^17 + 2^16 + 3: one combination, one sub-range combination, two leaves."""
    n = (1 << 17) + (1 << 16) + 3
    b = tiled(good512, n)
    got, st = eng.ecdsa_verify_recoverable_batch(*args(b), seed32=SEED, return_stats=True)
    assert got.all() and st["sub_combinations"] == 0 and st["verified_one_by_one"] == 0
    assert eng.ecdsa_batch_verify_rlc(*args(b)) is True
    bad = [0, 1 << 17, n - 1]
    for i in bad:
        b["digest"][i, 31] ^= 1
    expect = np.ones(n, np.uint8)
    expect[bad] = truth(oracle, b, bad)
    assert not expect[bad].any()
    assert eng.ecdsa_batch_verify_rlc(*args(b), seed32=SEED) is False
    got, st = eng.ecdsa_verify_recoverable_batch(*args(b), seed32=SEED, return_stats=True)
    assert np.array_equal(got, expect), np.nonzero(got != expect)[0][:10]
    assert st["sub_combinations"] > 0 and st["levels"] > 0 and not st["abandoned"]


def test_bisection_abandoned(eng, oracle, good512):
    """More than 8 failing ranges on one level end the bisection.  A level has 2^k ranges and only ranges above 2^17 items
    are split, so nine failing ranges need a fourth level: n > 2^20.  20 bad items, evenly spread, fail all 16 of them."""
    n = (1 << 20) + 11
    b = tiled(good512, n)
    bad = [k * (n // 20) + 3 for k in range(20)]
    for i in bad:
        b["digest"][i, 31] ^= 1
    expect = np.ones(n, np.uint8)
    expect[bad] = truth(oracle, b, bad)
    assert not expect[bad].any()
    got, st = eng.ecdsa_verify_recoverable_batch(*args(b), seed32=SEED, return_stats=True)
    assert np.array_equal(got, expect), np.nonzero(got != expect)[0][:10]
    assert st["abandoned"] and st["sub_combinations"] > 0


# ---- 7. refusals on the device ----
def test_refusals(eng, oracle, good512):
    b = tiled(good512, 16)
    lib, h = eng._lib, eng._h
    a = [x.ctypes.data for x in args(b)]
    seed = np.frombuffer(SEED, np.uint8)
    res = C.c_int(7)
    valid = np.full(16, 9, np.uint8)
    stats = np.full(4, 5, np.uint32)

    def rlc(n, ptrs, flags, seed_p=seed.ctypes.data, res_p=C.byref(res)):
        return lib.s2k_ecdsa_batch_verify_rlc(h, n, *ptrs, flags, seed_p, res_p)

    def bisect(n, ptrs, flags, seed_p=seed.ctypes.data, valid_p=valid.ctypes.data):
        return lib.s2k_ecdsa_verify_recoverable_batch_bisect(h, n, *ptrs, flags, seed_p, valid_p, stats.ctypes.data)

    for k in range(5):
        ptrs = list(a)
        ptrs[k] = None
        res.value = 7
        assert rlc(16, ptrs, 0) == ERR_ARG and res.value == 0
        assert bisect(16, ptrs, 0) == ERR_ARG
    assert rlc(16, a, 0, seed_p=None) == ERR_ARG and bisect(16, a, 0, seed_p=None) == ERR_ARG
    assert rlc(16, a, 0, res_p=None) == ERR_ARG and bisect(16, a, 0, valid_p=None) == ERR_ARG
    for flags in (2, 0x80000000, 0x40000001):
        assert rlc(16, a, flags) == ERR_ARG and bisect(16, a, flags) == ERR_ARG
    assert rlc(0x10000000, a, 0) == ERR_ARG and bisect(0x10000000, a, 0) == ERR_ARG
    d = [0x1000] * 5                                  # (never read: the device forms refuse before any launch)
    assert lib.s2k_ecdsa_batch_verify_rlc_device(h, 0x10000000, *d, 0, seed.ctypes.data, C.byref(res), None) == ERR_ARG
    assert lib.s2k_ecdsa_batch_verify_rlc_device(h, 16, None, *d[1:], 0, seed.ctypes.data, C.byref(res), None) == ERR_ARG
    assert lib.s2k_ecdsa_verify_recoverable_batch_bisect_device(h, 16, *d, 4, seed.ctypes.data, 0x1000, None, None) == ERR_ARG
    assert lib.s2k_ecdsa_verify_recoverable_batch_bisect_device(h, 16, *d, 0, seed.ctypes.data, None, None, None) == ERR_ARG
    assert (valid == 9).all() and (stats == 5).all()
    res.value = 0
    assert rlc(0, a, 0) == 0 and res.value == 1                                     # the empty batch
    check_both(eng, b, np.ones(16, np.uint8))


# ---- 8. the error point itself, under a given coefficient key (s2k_debug_ecdsa_rlc_point) ----
# The verdicts above are one bit per batch or per item; the value the bisection computes with is E = sum a_i E_i,
# E_i = R_i - u1_i G - u2_i Q_i, a_i by the item's index.  With the key given it is an exact group element: compared here with
# ecdsa_rlc_model.error_point over the oracle's arithmetic, in the aggregated form (0) and in the plain form's sub-ranges (1).
KEY = bytes(range(32, 64))


class PointModel:
    def __init__(self, oracle):
        import schnorr_rlc_model as SM
        self.ar, self.errors = SM.oracle_arith(oracle), {}

    def point(self, b, lo=0, cnt=None, reject=False):
        items = M.from_arrays(b)
        E, status = M.error_point(items, KEY, lo, cnt, ar=self.ar, reject_malleable=reject, errors=self.errors)
        flags = np.array([0 if M.checked_error(it, self.ar, reject, self.errors) is M.OUT else 1 for it in items], np.uint8)
        return pyref.enc65(E), status, flags


@pytest.fixture(scope="module")
def pm(oracle):
    return PointModel(oracle)


def check_point(eng, pm, b, reject=False):
    """both forms over the whole batch: the model's point, status and in-combination flags; returns the record"""
    want, status, flags = pm.point(b, reject=reject)
    any_out = not flags.all()
    assert status == any_out
    for form in (0, 1):
        res = eng.debug_ecdsa_rlc_point(*args(b), KEY, form, reject_malleable=reject)
        assert res["out"] == want, (form, res["out"].hex(), want.hex())
        assert (res["status"] != 0) == status, (form, res["status"])
        assert np.array_equal(res["in_comb"], flags), (form, np.nonzero(res["in_comb"] != flags)[0][:10])
    return want


def test_error_point_every_position_in_turn(eng, oracle, pm, good512):
    n = 257
    good = tiled(good512, n)
    assert check_point(eng, pm, good) == bytes(65)
    seen = set()
    for i in range(n):
        b = copy(good)
        b["digest"][i, 31 - i % 32] ^= 1 << (i % 8)
        want = check_point(eng, pm, b)
        assert want != bytes(65) and want not in seen, i
        seen.add(want)


@pytest.mark.parametrize("what", list(DAMAGES) + ["high s under the flag"])
def test_error_point_of_each_way_to_be_bad(eng, oracle, pm, good512, what):
    n, i = 300, 150
    b = tiled(good512, n)
    reject = what == "high s under the flag"
    if reject:
        put(b["s"], i, N - as_int(b["s"][i]))
        b["v"][i] ^= 1
    else:
        DAMAGES[what](b, i)
    assert truth(oracle, b, [i], reject)[0] == 0
    want = check_point(eng, pm, b, reject)
    out = not M.in_combination(*M.from_arrays(b)[i], reject_malleable=reject)
    assert (want == bytes(65)) == out, what            # left out: the status word alone rejects the batch


def test_error_point_of_sub_ranges(eng, oracle, pm, good512):
    n = 300
    b = tiled(good512, n)
    for i in (0, 149, 150, 299):
        b["digest"][i, 5] ^= 0x40
    put(b["r"], 77, 0)                                  # out of the combination
    whole, status, flags = pm.point(b)
    assert status and flags.sum() == n - 1 and whole != bytes(65)
    got = {}
    for lo, cnt in ((0, 150), (150, 150), (0, 1), (299, 1), (1, 298), (149, 2), (0, 300), (77, 1), (78, 71)):
        res = eng.debug_ecdsa_rlc_point(*args(b), KEY, 1, lo, cnt)
        want, in_range, _ = pm.point(b, lo, cnt)
        assert res["out"] == want, (lo, cnt)
        # the status word is the preparation's, over the whole batch: item 77 is out whether the range holds it or not
        assert res["status"] != 0 and in_range == (lo <= 77 < lo + cnt), (lo, cnt)
        assert np.array_equal(res["in_comb"], flags)
        got[lo, cnt] = res["out"]
    assert got[77, 1] == bytes(65) == got[78, 71]
    assert oracle.point_add(got[0, 150], got[150, 150]) == got[0, 300] == whole
    assert eng.debug_ecdsa_rlc_point(*args(b), KEY, 0)["out"] == whole
    put(b["r"], 77, as_int(tiled(good512, n)["r"][77]))
    assert eng.debug_ecdsa_rlc_point(*args(b), KEY, 1, 150, 150)["status"] == 0
