"""Whole-batch verification of BIP-340 signatures on the device (s2k_schnorr_batch_verify_rlc, s2k_schnorr_verify_batch_bisect)
against the big-integer model of schnorr_rlc_model.py, the error point exact.

The whole answer of the batch call is one bit, and a defect that takes an item out of the sum shows only when that very item
is bad.  s2k_debug_schnorr_rlc_point takes the coefficient key as given (KEY), so the error point of a rejected batch is a
predictable group element: E = sum a_i E_i with E_i = s_i G - lift_x(r_i) - e_i lift_x(pk_i).  Every expected point, status
and in-combination flag comes from the model, every expected verdict from oracle.schnorr_verify, never from the engine; all
comparisons are of bytes.  Large batches are a small oracle-checked batch tiled: a verdict and an error are functions of the
item alone, and the coefficients differ per index.

The status word the hook reads back is the preparation's, and the preparation runs over the whole batch: in form 1 it says
whether ANY item of the batch is out of the combination, whatever sub-range the point is of (asserted in test_sub_ranges).
"""
import ctypes as C
import random

import numpy as np
import pytest

import accept_corpus as AC
import pyref
import schnorr_rlc_model as M
from pyref import N, b32

pytestmark = pytest.mark.gpu

KEY = bytes(range(32, 64))
SEED = bytes(range(32))
ERR_ARG = -3
LENS = (0, 1, 31, 32, 33, 55, 56, 63, 64, 65, 119, 120, 200)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    return S.Engine(0)


class Ctx:
    """the model over the oracle's arithmetic, with every item's error and verdict computed once"""

    def __init__(self, oracle):
        self.oracle, self.ar = oracle, M.oracle_arith(oracle)
        self.errors, self.verdicts = M.Errors(self.ar), {}

    def truth(self, items):
        out = np.zeros(len(items), np.uint8)
        for k, it in enumerate(items):
            if it not in self.verdicts:
                self.verdicts[it] = 1 if self.oracle.schnorr_verify(*it) == 1 else 0
            out[k] = self.verdicts[it]
        return out

    def point(self, items, lo=0, cnt=None):
        return M.error_point(items, KEY, lo, cnt, ar=self.ar, errors=self.errors)

    def flags(self, items):
        return np.array([0 if self.errors(it) is M.OUT else 1 for it in items], np.uint8)


@pytest.fixture(scope="module")
def cx(oracle):
    return Ctx(oracle)


def hook(eng, items, form=0, lo=0, cnt=None):
    b = M.to_arrays(items)
    return eng.debug_schnorr_rlc_point(b["pk"], b["msgs"], b["sig"], KEY, form, lo, cnt)


def check_hook(eng, cx, items, forms=(0, 1)):
    """both forms of the hook over the whole batch: the model's point, status and flags; returns the point"""
    E, status = cx.point(items)
    flags = cx.flags(items)
    for form in forms:
        res = hook(eng, items, form)
        assert res["out"] == pyref.enc65(E), (form, res["out"].hex(), pyref.enc65(E).hex())
        assert (res["status"] != 0) == status, (form, res["status"])
        assert np.array_equal(res["in_comb"], flags), (form, np.nonzero(res["in_comb"] != flags)[0][:10])
    return E


def check_calls(eng, cx, items, seeds=(SEED, None)):
    """the whole-batch call says whether all are good; the bisect call gives the oracle's verdicts"""
    b = M.to_arrays(items)
    expect = cx.truth(items)
    for seed in seeds:
        assert eng.schnorr_batch_verify_rlc(b["pk"], b["msgs"], b["sig"], seed) is bool(expect.all())
    got = eng.schnorr_verify_batch_auto(b["pk"], b["msgs"], b["sig"], SEED)
    assert np.array_equal(got, expect), np.nonzero(got != expect)[0][:10]
    return expect


def check_all(eng, cx, items, forms=(0, 1)):
    E = check_hook(eng, cx, items, forms)
    expect = check_calls(eng, cx, items)
    assert (E is None and not cx.point(items)[1]) == bool(expect.all())      # the model and the oracle agree on the batch
    return E, expect


def flip_s(item, mask=1):
    return M.with_s(item, M.parts(item)[2] ^ mask)


def replaced(items, i, item):
    out = list(items)
    out[i] = item
    return out


@pytest.fixture(scope="module")
def good300(cx):
    """300 good items under 7 keys, messages of four lengths"""
    items = M.make_items(300, 7, seed=0x300, msg_lens=(32, 1, 33, 64), ar=cx.ar)
    assert cx.truth(items).all()
    return items


# ---- 1. good batches ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_good_batches(eng, cx, n):
    """messages of every length of LENS in one batch, through msg_offsets"""
    for nkeys in sorted({1, min(7, n), n}):
        items = M.make_items(n, nkeys, seed=1000 * n + nkeys, msg_lens=LENS[n % 13:] + LENS[:n % 13], ar=cx.ar)
        assert cx.truth(items).all()
        E, _ = check_all(eng, cx, items)
        assert E is None


@pytest.mark.parametrize("length", LENS)
def test_good_batches_fixed_message_length(eng, cx, length):
    """the same through a fixed msg_len and no offsets (length 0: no message buffer at all), straight through the C ABI"""
    n = 65
    items = M.make_items(n, 7, seed=0xF00 + length, msg_lens=(length,), ar=cx.ar)
    assert cx.truth(items).all()
    b = M.to_arrays(items)
    lib, h = eng._lib, eng._h
    msgs = np.frombuffer(b"".join(b["msgs"]) or b"\0", np.uint8)
    msgs_p = msgs.ctypes.data if length else None
    seed, key = np.frombuffer(SEED, np.uint8), np.frombuffer(KEY, np.uint8)

    def point(sig, form):
        out, status, flags = np.full(65, 9, np.uint8), C.c_uint32(5), np.full(n, 9, np.uint8)
        assert lib.s2k_debug_schnorr_rlc_point(h, n, b["pk"].ctypes.data, msgs_p, None, length, sig.ctypes.data, key.ctypes.data, form,
                                               0, n, out.ctypes.data, C.byref(status), flags.ctypes.data) == 0
        return out.tobytes(), status.value, flags

    for form in (0, 1):
        out, status, flags = point(b["sig"], form)
        assert out == bytes(65) and status == 0 and (flags == 1).all(), (form, length)
    res, valid = C.c_int(7), np.full(n, 9, np.uint8)
    assert lib.s2k_schnorr_batch_verify_rlc(h, n, b["pk"].ctypes.data, msgs_p, None, length, b["sig"].ctypes.data, seed.ctypes.data,
                                            C.byref(res)) == 0 and res.value == 1
    assert lib.s2k_schnorr_verify_batch_bisect(h, n, b["pk"].ctypes.data, msgs_p, None, length, b["sig"].ctypes.data, seed.ctypes.data,
                                               valid.ctypes.data, None) == 0 and (valid == 1).all()
    bad = b["sig"].copy()
    bad[n - 1, 63] ^= 1
    want = pyref.enc65(cx.point(replaced(items, n - 1, flip_s(items[n - 1])))[0])
    for form in (0, 1):
        assert point(bad, form)[0] == want != bytes(65), (form, length)


# ---- 2. every position in turn ----
def test_every_position_in_turn(eng, cx):
    """item i alone gets s ^= 1: the error point is a_i (+-G), for every i of 513 in the aggregated form (the full sweep:
    about 2 ms a call) and for every 8th i and the block borders in the plain form"""
    n = 513
    items = M.make_items(n, 7, seed=0x513, ar=cx.ar)
    assert cx.truth(items).all() and check_hook(eng, cx, items) is None
    plain = set(range(0, n, 8)) | {255, 256, 257, 511, 512}
    seen = set()
    for i in range(n):
        bad = replaced(items, i, flip_s(items[i]))
        E, status = cx.point(bad)
        sign = -1 if M.parts(items[i])[2] & 1 else 1                     # s ^ 1 = s - 1 or s + 1
        assert E == cx.ar.base_mult(sign * M.coefficient(KEY, i) % N) and not status
        seen.add(E)
        for form in (0, 1) if i in plain else (0,):
            res = hook(eng, bad, form)
            assert res["out"] == pyref.enc65(E), (i, form)
            assert res["status"] == 0 and res["in_comb"].all(), (i, form)
    assert len(seen) == n


# ---- 3. group shapes ----
GROUPS = (1, 2, 1023, 1024, 1025, 2500)          # one, two and three virtual groups of KG_VGROUP = 1024 members
SINGLETONS = 117


@pytest.fixture(scope="module")
def grouped(cx):
    """Key groups of the sizes of GROUPS and 117 further keys with one item each, in one fixed shuffled order.  The groups
    alone make 5575 items, so the batch has 5692, not 5200; 400 items are signed (2 + 60 + 60 + 60 + 100 for the five
    repeated keys, 118 singletons) and the groups are those tiled.  -> (items, members of every group, singleton positions)"""
    rng = random.Random(0x5200)
    keys = M.make_keys(len(GROUPS) + SINGLETONS, rng, cx.ar)
    signed = {1: 1, 2: 2, 1023: 60, 1024: 60, 1025: 60, 2500: 100}
    rows = []
    for g, size in enumerate(GROUPS + (1,) * SINGLETONS):
        d_even, pk, _ = keys[g]
        pool = []
        for _ in range(signed[size]):
            msg = rng.randbytes(rng.choice((32, 5, 70)))
            pool.append((pk, msg, M.sign(d_even, pk, msg, rng.randrange(1, N), cx.ar)))
        rows += [(g, pool[k % len(pool)]) for k in range(size)]
    assert len({it for _, it in rows}) == 400
    rng.shuffle(rows)
    items = [it for _, it in rows]
    members = [[i for i, (g, _) in enumerate(rows) if g == k] for k in range(len(GROUPS))]
    single = [i for i, (g, _) in enumerate(rows) if g >= len(GROUPS)]
    assert cx.truth(items).all() and len(items) == 5692 and [len(m) for m in members] == list(GROUPS)
    return items, members, single


@pytest.mark.parametrize("hash_bits", [0, 4])
def test_group_shapes(eng, cx, grouped, hash_bits):
    """hash_bits 4: a table of 16 slots for 123 keys, so most keys find no slot and their items are `left` items, each a
    lane of its own.  Which keys those are the grouping does not say: an item under each of 20 singleton keys is damaged,
    one call each."""
    import secp256k1_voi_amd as S
    items, members, single = grouped
    big = members[5]
    places = {"first of 2500": big[0], "last of 2500": big[-1], "1023rd of 2500": big[1022], "1024th of 2500": big[1023],
              "1025th of 2500": big[1024], "singleton group": members[0][0], "first of 1025": members[4][0],
              "last of 1025": members[4][-1]}
    places.update({f"singleton key {k}": single[5 * k] for k in range(20)})
    try:
        eng.set_key_grouping(S.KEYS_ADAPTIVE, hash_bits=hash_bits)
        E, _ = check_all(eng, cx, items)
        assert E is None
        for what, i in places.items():
            bad = replaced(items, i, flip_s(items[i], 1 << 9))
            E, expect = check_all(eng, cx, bad)
            assert E is not None and [int(j) for j in np.nonzero(expect == 0)[0]] == [i], what
        # a key that is no abscissa takes its whole group out of the combination (the key terms clear the flags)
        no_x = b32(M.first_non_abscissa())
        bad = [(no_x, it[1], it[2]) if k in set(members[3]) else it for k, it in enumerate(items)]
        E, expect = check_all(eng, cx, bad)
        assert E is None and int(expect.sum()) == len(items) - 1024
    finally:
        eng.set_key_grouping(S.KEYS_ADAPTIVE)


# ---- 4. each way to be bad ----
DAMAGE_NAMES = ("s = n", "s = n + 1", "s = 2^256 - 1", "a bit of s", "r = p", "r = p + 1", "r = a non-abscissa",
                "a bit of r that lifts", "a bit of r that does not lift", "pk = p", "pk = a non-abscissa",
                "pk = another valid key", "a bit of the message", "the message one byte shorter")


@pytest.mark.parametrize("what", DAMAGE_NAMES)
def test_each_way_to_be_bad(eng, cx, good300, what):
    for i in (0, 150, 299):
        bad = M.damages(good300, i)[what]
        E, expect = check_all(eng, cx, bad)
        assert [int(j) for j in np.nonzero(expect == 0)[0]] == [i], (what, i)
        out = cx.errors(bad[i]) is M.OUT
        assert (E is None) == out                   # left out: nothing of it in the sum, the status word alone rejects


def corpus_items(c):
    return [(bytes(c["pk32"][i]), bytes(c["msgs"][i]), bytes(c["sig"][i])) for i in range(len(c["cls"]))]


def test_accept_corpus_as_one_batch(eng, cx, oracle):
    """2 valid items, 512 flips of a bit of r on a fixed R, the 2 odd-y twins and 90 fillers in one batch"""
    c = AC.corpus(oracle)["schnorr"]
    items = corpus_items(c)
    assert len(items) == 606
    E, expect = check_all(eng, cx, items)
    assert E is not None and np.array_equal(expect, c["exp"])


def test_accept_corpus_members_in_turn(eng, cx, oracle):
    """Among the fillers, every rejected member takes the place of its valid parent: the odd-y twins one at a time (s G - e P
    is -R there, so the error is -2 a_i R_i, not the identity), the bit flips sixteen to a call, each at a place of its own
    (the parent's and fifteen fillers')."""
    c = AC.corpus(oracle)["schnorr"]
    items = corpus_items(c)
    base = [i for i, k in enumerate(c["cls"]) if k in AC.BIP_VALID_CLASSES]
    batch = [items[i] for i in base]
    assert len(batch) == 92 and cx.truth(batch).all() and check_hook(eng, cx, batch) is None
    where = {i: k for k, i in enumerate(base)}
    for t in (i for i, k in enumerate(c["cls"]) if k == AC.BIP_ODD):
        at = where[int(c["parent"][t])]
        bad = replaced(batch, at, items[t])
        E, expect = check_all(eng, cx, bad)
        R = pyref.lift_x(M.parts(items[t])[1], 0)
        assert E == cx.ar.mul(-2 * M.coefficient(KEY, at) % N, R) and E is not None
        assert [int(j) for j in np.nonzero(expect == 0)[0]] == [at]
    flips = [i for i, k in enumerate(c["cls"]) if k == AC.BIP_BIT]
    assert len(flips) == 512
    fillers = [k for k, i in enumerate(base) if c["cls"][i] == AC.BIP_FILLER]
    for g in range(0, 512, 16):
        bad = list(batch)
        places = [where[int(c["parent"][flips[g]])]] + fillers[g % 75:g % 75 + 15]
        for f, at in zip(flips[g:g + 16], places):
            bad[at] = items[f]
        E, expect = check_all(eng, cx, bad)
        assert sorted(int(j) for j in np.nonzero(expect == 0)[0]) == sorted(places)


# ---- 5. the cancelling pair ----
@pytest.mark.parametrize("at", [(0, 1), (1, 2), (255, 256), (10, 17)])
def test_cancelling_pair(eng, cx, good300, at):
    """(r_i, s_i + d) and (r_j, s_j - d): the errors are d G and -d G, equal coefficients would cancel them.  (10, 17): two
    members of one key group (7 keys, item i under key i mod 7)."""
    i, j = at
    assert at != (10, 17) or good300[10][0] == good300[17][0]
    delta = random.Random(0xCA + i).randrange(1, N)
    p1, p2 = M.cancelling_pair(good300[i], good300[j], delta)
    bad = replaced(replaced(good300, i, p1), j, p2)
    E = check_hook(eng, cx, bad)
    assert E is not None and E == cx.ar.base_mult((M.coefficient(KEY, i) - M.coefficient(KEY, j)) * delta % N)
    expect = check_calls(eng, cx, bad, seeds=(SEED, bytes(range(1, 33))))
    assert [int(k) for k in np.nonzero(expect == 0)[0]] == [i, j]


# ---- 6. exceptional points in the sum ----
def test_exceptional_points(eng, cx):
    items = M.exceptional_items(6, cx.ar)
    assert cx.truth(items).all()
    E, _ = check_all(eng, cx, items)
    assert E is None
    for i in (17, 65, 68):
        pk, msg, sig = items[i]
        bad = replaced(items, i, (pk, bytes([msg[0] ^ 0x80]) + msg[1:], sig))
        E, expect = check_all(eng, cx, bad)
        assert E is not None and [int(j) for j in np.nonzero(expect == 0)[0]] == [i]
    # all 64 copies of the repeated signature damaged alike: 64 equal errors under 64 coefficients
    pk, msg, sig = items[0]
    bad = [(pk, bytes([msg[0] ^ 1]) + msg[1:], sig) if k < 64 else it for k, it in enumerate(items)]
    E, expect = check_all(eng, cx, bad)
    assert E is not None and not expect[:64].any() and expect[64:].all()


# ---- 7. sub-ranges ----
def test_sub_ranges(eng, cx, good300, oracle):
    n = 300
    bad = list(good300)
    for i in (0, 149, 150, 299):
        bad[i] = flip_s(good300[i], 1 << (i % 200))
    bad[77] = M.damages(good300, 77)["r = a non-abscissa"][77]
    whole, status = cx.point(bad)
    assert status and whole is not None
    got = {}
    for lo, cnt in ((0, 150), (150, 150), (0, 1), (299, 1), (1, 298), (149, 2), (0, 300), (77, 1), (78, 71)):
        res = hook(eng, bad, 1, lo, cnt)
        E, in_range = cx.point(bad, lo, cnt)
        assert res["out"] == pyref.enc65(E), (lo, cnt)
        # the status word is the preparation's: item 77 is out of the combination, whether the range holds it or not
        assert res["status"] != 0 and in_range == (lo <= 77 < lo + cnt), (lo, cnt)
        assert np.array_equal(res["in_comb"], cx.flags(bad)) and res["in_comb"].sum() == n - 1
        got[lo, cnt] = res["out"]
    assert got[77, 1] == bytes(65) == got[78, 71]
    assert oracle.point_add(got[0, 150], got[150, 150]) == got[0, 300] == pyref.enc65(whole)
    assert hook(eng, bad, 0)["out"] == got[0, 300]
    # without the item that is out, the status word is 0 in both forms
    ok = replaced(bad, 77, good300[77])
    assert hook(eng, ok, 1, 150, 150)["status"] == 0 and hook(eng, ok, 0)["status"] == 0


# ---- 8. bisection past a leaf, with an odd split ----
def test_bisection_past_a_leaf(eng, cx):
    """Ranges of up to 2^17 items are leaves.  n = 2^17 + 2^16 + 3 splits into 98305 and 98306: one combination, one sub-range
    combination (k_rlc_save, k_rlc_gather and the sum on a sub-range with the batch's stride), two leaves."""
    n = (1 << 17) + (1 << 16) + 3
    base = M.make_items(512, 7, seed=0x8512, ar=cx.ar)
    assert cx.truth(base).all()
    items = (base * (n // 512 + 1))[:n]
    b = M.to_arrays(base)
    pk, sig = np.resize(b["pk"], (n, 32)), np.resize(b["sig"], (n, 64))
    msgs = np.resize(np.frombuffer(b"".join(b["msgs"]), np.uint8).reshape(512, 32), (n, 32))
    got, st = eng.schnorr_verify_batch_auto(pk, msgs, sig, SEED, return_stats=True)
    assert got.all() and st["sub_combinations"] == 0 and st["verified_one_by_one"] == 0
    assert eng.schnorr_batch_verify_rlc(pk, msgs, sig, SEED) is True
    where = [0, n // 2 - 1, n // 2, n - 1]
    for i in where:
        sig[i, 63] ^= 1
        items[i] = flip_s(items[i])
    expect = cx.truth(items)
    assert [int(i) for i in np.nonzero(expect == 0)[0]] == where
    assert eng.schnorr_batch_verify_rlc(pk, msgs, sig, SEED) is False
    got, st = eng.schnorr_verify_batch_auto(pk, msgs, sig, SEED, return_stats=True)
    assert np.array_equal(got, expect), np.nonzero(got != expect)[0][:10]
    assert st["sub_combinations"] > 0 and st["levels"] > 0 and not st["abandoned"]
    # the halves as the bisection cuts them, and the whole: the model's points
    for form, lo, cnt in ((1, 0, n // 2), (1, n // 2, n - n // 2), (0, 0, n)):
        res = eng.debug_schnorr_rlc_point(pk, msgs, sig, KEY, form, lo, cnt)
        assert res["out"] == pyref.enc65(cx.point(items, lo, cnt)[0]) != bytes(65), (form, lo)
        assert res["status"] == 0 and res["in_comb"].all()


# ---- 9. device forms ----
def test_device_forms(eng, cx):
    import torch
    n = 257
    items = M.make_items(n, 7, seed=0x9257, ar=cx.ar)
    assert cx.truth(items).all()
    lib, h = eng._lib, eng._h
    seed = np.frombuffer(SEED, np.uint8)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0

    def run(items):
        b = M.to_arrays(items)
        msgs = np.frombuffer(b"".join(b["msgs"]), np.uint8).reshape(n, 32)
        dev = [torch.from_numpy(a.copy()).cuda() for a in (b["pk"], msgs, b["sig"])]
        valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res, stats = C.c_int(7), np.full(4, 5, np.uint32)
        assert lib.s2k_schnorr_batch_verify_rlc_device(h, n, dev[0].data_ptr(), dev[1].data_ptr(), None, 32, dev[2].data_ptr(),
                                                       seed.ctypes.data, C.byref(res), stream.cuda_stream) == 0
        assert lib.s2k_schnorr_verify_batch_bisect_device(h, n, dev[0].data_ptr(), dev[1].data_ptr(), None, 32, dev[2].data_ptr(),
                                                          seed.ctypes.data, valid.data_ptr(), stats.ctypes.data, stream.cuda_stream) == 0
        stream.synchronize()
        return res.value, valid.cpu().numpy()

    verdict, valid = run(items)
    assert verdict == 1 and np.array_equal(valid, np.ones(n, np.uint8))
    bad = replaced(items, 200, flip_s(items[200]))
    verdict, valid = run(bad)
    expect = cx.truth(bad)
    assert verdict == 0 and expect[200] == 0 and expect.sum() == n - 1 and np.array_equal(valid, expect)


# ---- 10. refusals ----
def test_refusals(eng, cx):
    n = 16
    items = M.make_items(n, 3, seed=0x10, ar=cx.ar)
    assert cx.truth(items).all()
    b = M.to_arrays(items)
    msgs = np.frombuffer(b"".join(b["msgs"]), np.uint8)
    lib, h = eng._lib, eng._h
    seed, key = np.frombuffer(SEED, np.uint8), np.frombuffer(KEY, np.uint8)
    res = C.c_int(7)
    valid, stats = np.full(n, 9, np.uint8), np.full(4, 5, np.uint32)
    pk, sig = b["pk"].ctypes.data, b["sig"].ctypes.data

    def rlc(pk=pk, msgs=msgs.ctypes.data, msg_len=32, sig=sig, seed_p=seed.ctypes.data, res_p=C.byref(res)):
        res.value = 7
        return lib.s2k_schnorr_batch_verify_rlc(h, n, pk, msgs, None, msg_len, sig, seed_p, res_p)

    def bisect(pk=pk, msgs=msgs.ctypes.data, msg_len=32, sig=sig, seed_p=seed.ctypes.data, valid_p=valid.ctypes.data):
        return lib.s2k_schnorr_verify_batch_bisect(h, n, pk, msgs, None, msg_len, sig, seed_p, valid_p, stats.ctypes.data)

    for kw in ({"pk": None}, {"sig": None}, {"msgs": None}, {"msg_len": 0x80000000}, {"msg_len": 1 << 40}):
        assert rlc(**kw) == ERR_ARG and res.value == 0, kw
        assert bisect(**kw) == ERR_ARG, kw
    assert rlc(seed_p=None) == ERR_ARG and bisect(seed_p=None) == ERR_ARG
    assert rlc(res_p=None) == ERR_ARG and bisect(valid_p=None) == ERR_ARG
    assert (valid == 9).all()
    d = 0x1000                                           # (never read: the device forms refuse before any launch)
    for kw in ({"pk": None}, {"sig": None}, {"msgs": None}, {"msg_len": 0x80000000}, {"n": 0x10000000}):
        a = {"n": n, "pk": d, "msgs": d, "msg_len": 32, "sig": d}
        a.update(kw)
        res.value = 7
        assert lib.s2k_schnorr_batch_verify_rlc_device(h, a["n"], a["pk"], a["msgs"], None, a["msg_len"], a["sig"], seed.ctypes.data,
                                                       C.byref(res), None) == ERR_ARG and res.value == 0, kw
        assert lib.s2k_schnorr_verify_batch_bisect_device(h, a["n"], a["pk"], a["msgs"], None, a["msg_len"], a["sig"], seed.ctypes.data,
                                                          d, None, None) == ERR_ARG, kw
    assert lib.s2k_schnorr_batch_verify_rlc_device(h, n, d, d, None, 32, d, None, C.byref(res), None) == ERR_ARG
    assert lib.s2k_schnorr_batch_verify_rlc_device(h, n, d, d, None, 32, d, seed.ctypes.data, None, None) == ERR_ARG
    assert lib.s2k_schnorr_verify_batch_bisect_device(h, n, d, d, None, 32, d, seed.ctypes.data, None, None, None) == ERR_ARG

    # the hook's own refusals
    out, status, flags = np.full(65, 9, np.uint8), C.c_uint32(5), np.full(n, 9, np.uint8)

    def point(n=n, pk=pk, msgs=msgs.ctypes.data, msg_len=32, sig=sig, key_p=key.ctypes.data, form=0, lo=0, cnt=n, out_p=out.ctypes.data,
              status_p=C.byref(status), flags_p=flags.ctypes.data):
        return lib.s2k_debug_schnorr_rlc_point(h, n, pk, msgs, None, msg_len, sig, key_p, form, lo, cnt, out_p, status_p, flags_p)

    for kw in ({"pk": None}, {"sig": None}, {"msgs": None}, {"key_p": None}, {"out_p": None}, {"status_p": None},
               {"msg_len": 0x80000000}, {"n": 0, "cnt": 0}, {"n": (1 << 22) + 1, "cnt": (1 << 22) + 1},
               {"form": 2}, {"form": -1}, {"form": 0, "lo": 1, "cnt": n - 1}, {"form": 0, "cnt": n - 1}, {"form": 0, "cnt": n + 1},
               {"form": 1, "cnt": 0}, {"form": 1, "lo": n, "cnt": 1}, {"form": 1, "lo": 1, "cnt": n}, {"form": 1, "cnt": n + 1},
               {"form": 1, "lo": (1 << 64) - 1, "cnt": 2}, {"form": 1, "lo": 2, "cnt": (1 << 64) - 1}):
        assert point(**kw) == ERR_ARG, kw
    assert (out == 9).all() and status.value == 5 and (flags == 9).all()
    assert point(form=1, lo=n - 1, cnt=1, flags_p=None) == 0 and status.value == 0 and not out.any()

    # a good call afterwards still answers
    assert rlc() == 0 and res.value == 1
    assert bisect() == 0 and valid.all()
    E, _ = check_all(eng, cx, items)
    assert E is None
