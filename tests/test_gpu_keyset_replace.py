"""Replacing and removing keys of a key set in place (s2k_keyset_replace[_device], s2k_keyset_remove): after every call the set
is, in every call that takes it, the set created whole from the changed key list - verdicts by index (small call and lane
path, ECDSA and BIP-340), by key bytes and encoded, valid_keys(), the three lookups and the index's occupied count - with the
oracle as the truth of the verdicts and a dictionary as the truth of the lookups.

The set has 200 keys, the shapes of tests/test_gpu_keyset_append.py: no section of such a set is a multiple of 256 bytes
long, and the slots replaced are the first, the last, a run across the 64-lane block given out of order, 37 scattered ones in
pieces of 16 (three pieces, the last of five), all 200 in pieces of 64 (the last of eight), 11 removed and five of them
filled again, and - on the set with spare capacity - rows that an append made.

Keys and signatures.  A row holds an ECDSA key ("E", signs the ECDSA batch) or a lifted BIP-340 key ("S", signs the BIP-340
batch), or one of: an E key off the curve, one with X >= p, the all-zero key, the negation of an S key held elsewhere (same x:
its BIP-340 signatures verify under it too).  Every signature is made by one key and names a slot that key lives in at some
step: it is false before the key arrives, true while it is there, false after it left - both directions are asserted.  Slot 60
starts as a duplicate of slot 5; slot 5 is replaced and the 64-byte lookup of the old bytes must then answer 60."""
import os

import numpy as np
import pytest

import pyref as R

pytestmark = pytest.mark.gpu
P = R.P
b32 = R.b32
NONE = 0xFFFFFFFF
ROW_DEFAULT, QUAD_DEFAULT = 3072, 32768
NKEYS, SPARE_CAP, NAPPEND = 200, 264, 27
NROW, NSIG = 300, 4096 + 37
LAYOUTS = ["KEYSET_CHUNKS", "KEYSET_JOINT", "KEYSET_JOINT5", "KEYSET_JOINT6", "KEYSET_COMB"]
PERM = np.random.default_rng(2401).permutation(NKEYS)
SCATTER = [int(x) for x in PERM[:37]]
REMOVED = [int(x) for x in np.random.default_rng(2402).permutation(NKEYS)[:11]]


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


def _negated(key):
    out = key.copy()
    out[32:] = np.frombuffer(b32(P - int.from_bytes(bytes(key[32:]), "big")), np.uint8)
    return out


def _lift_even(x32):
    x = int.from_bytes(bytes(x32), "big")
    y = pow((x * x * x + 7) % P, (P + 1) // 4, P)
    assert y * y % P == (x * x * x + 7) % P
    return np.frombuffer(bytes(x32) + b32(y if y % 2 == 0 else P - y), np.uint8)


def _corrupt(rng, arrays, n):
    """a bit of one of the arrays changed in about a quarter of the n rows"""
    hit = rng.permutation(n)[:n // 4]
    for arr, part in zip(arrays, np.array_split(hit, len(arrays))):
        arr[part, rng.integers(0, arr.shape[1], size=part.size)] ^= (1 << rng.integers(0, 8, size=part.size)).astype(np.uint8)
    clean = np.ones(n, bool)
    clean[hit] = False
    return clean


# ---- the schedule: which key every row holds after every step (no device, no randomness beyond the fixed permutations) ----
def _schedule():
    """(initial rows, steps).  A row is ("E", id) / ("S", id) / ("Eoff", id) / ("Ebig", id) / ("Sneg", id) / ("ZERO",); a step is
    dict(op, slots, rows, piece, spare) - op "replace" / "replace_device" / "remove" / "append"; spare: only on the set with spare
    capacity."""
    count = {"E": 0, "S": 0}

    def new(kind):
        count[kind[0]] += 1
        return (kind, count[kind[0]] - 1)

    def fresh(slots):
        return [new("E" if i % 2 == 0 else "S") for i in range(len(slots))]

    rows = [new("E" if i % 2 == 0 else "S") for i in range(NKEYS)]
    rows[60] = rows[5]                                       # a duplicate at a higher slot, from the start
    initial = list(rows)
    steps = []

    def step(op, slots, new_rows, piece=0, spare=False):
        steps.append(dict(op=op, slots=list(slots), rows=list(new_rows), piece=piece, spare=spare))
        if op == "append":
            rows.extend(new_rows)
        else:
            for s, r in zip(slots, new_rows):
                rows[s] = r

    step("replace", [0], [new("E")])                                          # 1. the first row
    step("replace", [199], [new("S")])                                        # 2. the last live row
    step("replace_device", [65, 63, 64], [new("E"), new("Eoff"), new("S")])   # 3. across the 64-lane block, out of order
    step("replace", [5], [new("S")])                                          #    the re-election: its duplicate lives on at 60
    # 4. 37 scattered slots in pieces of 16; among the keys: X >= p, all zero, the negation of an S key still held, a
    # duplicate of a key still held at a higher slot and one of a key still held at a lower slot
    sc = sorted(SCATTER)
    held = [s for s in range(NKEYS) if s not in SCATTER and s not in (5, 60)]
    held_s = [s for s in held if rows[s][0] == "S"]
    new4 = dict(zip(SCATTER, fresh(SCATTER)))
    new4[sc[0]] = rows[held[-1]]                             # lowest slot of the call <- the key of a higher held slot
    new4[sc[-1]] = rows[held[0]]                             # highest slot of the call <- the key of a lower held slot
    new4[sc[1]] = ("Sneg", rows[held_s[3]][1])
    new4[sc[2]] = new("Ebig")
    new4[sc[3]] = ("ZERO",)
    assert sc[0] < held[-1] and sc[-1] > held[0]
    step("replace", SCATTER, [new4[s] for s in SCATTER], piece=16)
    # 5. every row in pieces of 64: fresh keys, two rows of one new key, bad keys again
    allslots = [int(x) for x in PERM[::-1]]
    new5 = dict(zip(allslots, fresh(allslots)))
    new5[60] = new5[5]
    new5[100] = new("Eoff")
    new5[150] = new("Ebig")
    new5[130] = ("Sneg", next(new5[t][1] for t in range(10, 50) if new5[t][0] == "S"))
    step("replace", allslots, [new5[s] for s in allslots], piece=64)
    # 6. 11 rows removed, five of them filled again
    step("remove", REMOVED, [("ZERO",)] * len(REMOVED))
    step("replace", REMOVED[2:7], fresh(REMOVED[2:7]))
    # 7. replace composes with append: rows an append made are replaced like any other
    step("append", range(NKEYS, NKEYS + NAPPEND), fresh(range(NAPPEND)), spare=True)
    step("replace", [NKEYS + NAPPEND - 1, NKEYS + 10, 3], [new("S"), new("E"), new("E")], spare=True)
    return initial, steps, count["E"], count["S"]


def _places(initial, steps):
    """per signing key, the slots it lives in at some step (an E key off the curve counts: its signatures stay false)"""
    where = {}
    for slot, row in list(enumerate(initial)) + [(s, r) for st in steps for s, r in zip(st["slots"], st["rows"])]:
        if row[0] != "ZERO" and row[0] != "Ebig":
            where.setdefault((row[0][0], row[1]), [])
            if slot not in where[(row[0][0], row[1])]:
                where[(row[0][0], row[1])].append(slot)
    return where


@pytest.fixture(scope="module")
def case(eng, oracle):
    """The keys, both signature batches, and after every step: the key list, its validity, the oracle's verdicts for both
    batches, the arguments of the call by key bytes and of the encoded call.  Computed once for all layouts."""
    from secp256k1_voi_amd.synth import synth_batch, synth_schnorr_batch
    initial, steps, UE, US = _schedule()
    where = _places(initial, steps)
    j = np.arange(NSIG)
    pubE, dig, r, s = (np.array(a) for a in synth_batch(eng, NSIG, UE, seed=2411, key_idx=j % UE))
    pk, msgs, sig = (np.array(a) for a in synth_schnorr_batch(eng, NSIG, US, seed=2412))
    QE, QS = pubE[:UE], np.stack([_lift_even(x) for x in pk[:US]])
    # signature i, made by key i mod U, names one of the slots that key lives in (a key no row ever holds: a slot of the other kind)
    kidx_e = np.array([where.get(("E", i % UE), [1])[(i // UE) % len(where.get(("E", i % UE), [1]))] for i in j], np.uint32)
    kidx_s = np.array([where.get(("S", i % US), [2])[(i // US) % len(where.get(("S", i % US), [2]))] for i in j], np.uint32)
    clean_e = _corrupt(np.random.default_rng(2413), (r, s, dig), NSIG)
    clean_s = _corrupt(np.random.default_rng(2414), (sig, msgs), NSIG)

    def key_of(row):
        if row[0] == "ZERO":
            return np.zeros(64, np.uint8)
        if row[0] in ("S", "Sneg"):
            return QS[row[1]] if row[0] == "S" else _negated(QS[row[1]])
        k = QE[row[1]].copy()
        if row[0] == "Eoff":
            k[63] ^= 1
        if row[0] == "Ebig":
            k[:32] = np.frombuffer(b32(P + 5), np.uint8)
        return k

    schnorr_cache = {}

    def state(rows):
        n = len(rows)
        keys = np.stack([key_of(x) for x in rows])
        valid = np.array([x[0] in ("E", "S", "Sneg") for x in rows], np.uint8)
        padded = np.concatenate([keys, np.zeros((SPARE_CAP + 1 - n, 64), np.uint8)])      # an index >= n names no key
        pub = np.ascontiguousarray(padded[kidx_e])
        truth_e = np.where(kidx_e < n, oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=os.cpu_count() or 1), 0).astype(np.uint8)
        truth_s = np.zeros(NSIG, np.uint8)
        for i in range(NSIG):
            k = int(kidx_s[i])
            if k < n and valid[k]:
                key = (i, bytes(keys[k, :32]))
                if key not in schnorr_cache:
                    schnorr_cache[key] = int(bool(oracle.schnorr_verify(key[1], bytes(msgs[i]), bytes(sig[i]))))
                truth_s[i] = schnorr_cache[key]
        pvalid = np.concatenate([valid, np.zeros(SPARE_CAP + 1 - n, np.uint8)])[kidx_e]
        pubs = [bytes([2 + (int(q[63]) & 1)]) + bytes(q[:32]) if v else b"\x04" + bytes(q) for q, v in zip(pub, pvalid)]
        return dict(rows=list(rows), n=n, keys=keys, valid=valid, pub=pub, pubs=pubs, truth_e=truth_e, truth_s=truth_s)

    rows = list(initial)
    states = {False: [state(rows)], True: [state(rows)]}     # (by `spare`: the set without spare capacity skips the steps of 7)
    for st in steps:
        if st["op"] == "append":
            rows = rows + st["rows"]
        else:
            rows = list(rows)
            for slot, row in zip(st["slots"], st["rows"]):
                rows[slot] = row
        st["keys"] = np.stack([key_of(x) for x in st["rows"]])
        states[True].append(state(rows))
        if not st["spare"]:
            states[False].append(states[True][-1])
    first = states[True][0]
    assert np.array_equal(eng.ecdsa_verify_batch(first["pub"], dig, r, s), first["truth_e"])
    assert 0.2 * NSIG < int(first["truth_e"].sum()) < 0.6 * NSIG and 0.2 * NSIG < int(first["truth_s"].sum()) < 0.6 * NSIG
    allkeys = np.unique(np.concatenate([st["keys"] for st in states[True]]), axis=0)
    queries = np.ascontiguousarray(np.concatenate([allkeys, np.stack([_negated(k) for k in allkeys])]))
    return dict(steps=steps, states=states, kidx_e=kidx_e, kidx_s=kidx_s, dig=dig, r=r, s=s, msgs=msgs, sig=sig, clean_e=clean_e, clean_s=clean_s,
                queries=queries, digs=[bytes(d) for d in dig], sigs=[bytes(a) + bytes(b) for a, b in zip(r, s)])


def _lookup_truth(keys, valid, live, q):
    """the answers of the three lookups for the 64-byte queries q over keys[:live]: the lowest index"""
    d64, d32, d33 = {}, {}, {}
    for i in range(live):
        k = bytes(keys[i])
        d64.setdefault(k, i)
        d32.setdefault(k[:32], i)
        if valid[i]:
            d33.setdefault((k[63] & 1, k[:32]), i)
    e64 = np.array([d64.get(bytes(k), NONE) for k in q], np.uint32)
    e32 = np.array([d32.get(bytes(k[:32]), NONE) for k in q], np.uint32)
    e33 = np.array([d33.get((int(k[63]) & 1, bytes(k[:32])), NONE) for k in q], np.uint32)
    return e64, e32, e33, len(d64)


def _check_index(eng, ks, st, queries):
    e64, e32, e33, distinct = _lookup_truth(st["keys"], st["valid"], st["n"], queries)
    assert np.array_equal(eng.keyset_lookup(ks, queries), e64)
    assert np.array_equal(eng.keyset_lookup(ks, queries, key_bytes=32, stride=64), e32)
    rec33 = np.ascontiguousarray(np.concatenate([(2 + (queries[:, 63:64] & 1)).astype(np.uint8), queries[:, :32]], axis=1))
    assert np.array_equal(eng.keyset_lookup(ks, rec33, key_bytes=33), e33)
    assert ks.index_info()["occupied"] == distinct


def _by_index(eng, S, ks, c):
    """the verdicts by index: ECDSA small call and whole batch, BIP-340 whole batch"""
    comb = ks.layout() == S.KEYSET_COMB
    small = eng.ecdsa_verify_batch_keyset(ks, c["kidx_e"][:NROW], c["dig"][:NROW], c["r"][:NROW], c["s"][:NROW])
    assert eng.last_keyset_ladder() == (S.KEYSET_LADDER_LANE if comb else S.KEYSET_LADDER_ROW)
    full = eng.ecdsa_verify_batch_keyset(ks, c["kidx_e"], c["dig"], c["r"], c["s"])
    assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
    return small, full, eng.schnorr_verify_batch_keyset(ks, c["kidx_s"], c["msgs"], c["sig"])


def _check_all(eng, S, ks, c, st, layout, cap, indexed=True):
    """everything the contract names, against the oracle, the dictionary and a set created whole from the list"""
    n = st["n"]
    assert len(ks) == n and ks.capacity() == cap and ks.layout() == layout
    assert np.array_equal(ks.valid_keys(), st["valid"])
    small, full, schnorr = _by_index(eng, S, ks, c)
    assert np.array_equal(small, st["truth_e"][:NROW]), np.nonzero(small != st["truth_e"][:NROW])[0][:10]
    assert np.array_equal(full, st["truth_e"]), np.nonzero(full != st["truth_e"])[0][:10]
    assert np.array_equal(schnorr, st["truth_s"]), np.nonzero(schnorr != st["truth_s"])[0][:10]
    whole = eng.keyset_create(st["keys"], layout, capacity=cap)
    try:
        assert np.array_equal(whole.valid_keys(), st["valid"])
        for got, ref in zip((small, full, schnorr), _by_index(eng, S, whole, c)):
            assert np.array_equal(got, ref)
    finally:
        whole.close()
    if layout == S.KEYSET_COMB:
        # the wave-per-signature ladder over the comb tables reads the replaced rows too
        eng.set_keyset_comb_small_batch_max(2048)
        try:
            got = eng.ecdsa_verify_batch_keyset(ks, c["kidx_e"][:NROW], c["dig"][:NROW], c["r"][:NROW], c["s"][:NROW])
            assert eng.last_keyset_ladder() == S.KEYSET_LADDER_ROW_COMB and np.array_equal(got, st["truth_e"][:NROW])
        finally:
            eng.set_keyset_comb_small_batch_max(0)
    if not indexed:
        return
    _check_index(eng, ks, st, c["queries"])
    got = eng.ecdsa_verify_batch_bykey(ks, st["pub"], c["dig"], c["r"], c["s"])
    assert np.array_equal(got, st["truth_e"]) and eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE
    got = eng.ecdsa_verify_encoded_batch_keyset(ks, st["pubs"], c["digs"], c["sigs"], encoding=S.ENCODING_COMPACT)
    assert np.array_equal(got, st["truth_e"])


def _apply(S, ks, step):
    import torch
    S.debug_keyset_replace_piece(step["piece"])
    try:
        slots = np.array(step["slots"], np.uint32)
        if step["op"] == "replace":
            ks.replace(slots, step["keys"])
        elif step["op"] == "replace_device":
            ks.replace(slots, torch.from_numpy(step["keys"]).to(torch.device("cuda", 0)))
        elif step["op"] == "remove":
            ks.remove(slots)
        else:
            assert ks.append(step["keys"]) == step["slots"][0]
    finally:
        S.debug_keyset_replace_piece(0)


def _flips(c, before, after, slots):
    """clean signatures that went true -> false and false -> true; nothing outside `slots` moved"""
    down = up = 0
    for kidx, clean, t in ((c["kidx_e"], c["clean_e"], "truth_e"), (c["kidx_s"], c["clean_s"], "truth_s")):
        moved = before[t] != after[t]
        assert np.isin(kidx[moved], slots).all()
        down += int((clean & moved & (before[t] == 1)).sum())
        up += int((clean & moved & (after[t] == 1)).sum())
    return down, up


# ---- 1. the sequence, on every layout, with and without spare capacity ----
@pytest.mark.parametrize("spare,log2_slots", [(False, 0), (True, 9)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_replace_sequence(eng, case, layout, spare, log2_slots):
    import ctypes as C
    import secp256k1_voi_amd as S
    c, layout = case, getattr(S, layout)
    cap = SPARE_CAP if spare else NKEYS
    states = c["states"][spare]
    steps = [st for st in c["steps"] if spare or not st["spare"]]
    ks = eng.keyset_create(states[0]["keys"], layout, capacity=cap)
    eng.set_small_batch_max(0)           # (the call by key bytes and the encoded call are not to delegate to the plain ladders)
    eng.set_mid_batch_max(0)
    try:
        ks.index_create(log2_slots)
        slots_before = ks.index_info()["slots"]
        assert slots_before == 512
        _check_all(eng, S, ks, c, states[0], layout, cap)
        for i, step in enumerate(steps):
            _apply(S, ks, step)
            _check_all(eng, S, ks, c, states[i + 1], layout, cap)
            assert ks.index_info()["slots"] == slots_before              # the geometry the index had
            if step["op"] != "append":
                down, up = _flips(c, states[i], states[i + 1], step["slots"])
                # signatures of the old keys turned false, those of the new keys true: at least five clean ones each
                # (rows that held no key have no signatures to lose, rows that get none have none to win)
                held = states[i]["valid"][step["slots"]].any()
                assert (down >= 5 if held else down == 0) and (up >= 5 if step["op"] != "remove" else up == 0), (i, down, up)
            if step["slots"] == [5]:
                old = states[i]["keys"][5:6]
                assert eng.keyset_lookup(ks, old).tolist() == [60]          # the duplicate was re-elected
        last = states[len(steps)]
        n = last["n"]
        # refusals: nothing is touched
        key = last["keys"][:2].copy()
        for bad in ([n], [cap], [3, n], [7, 7], [7, 150, 3, 7]):
            with pytest.raises(S.EngineError):
                ks.replace(np.array(bad, np.uint32), key[:1].repeat(len(bad), axis=0))
            with pytest.raises(S.EngineError):
                ks.remove(np.array(bad, np.uint32))
            full = eng.ecdsa_verify_batch_keyset(ks, c["kidx_e"], c["dig"], c["r"], c["s"])
            assert np.array_equal(full, last["truth_e"]) and np.array_equal(ks.valid_keys(), last["valid"])
            _check_index(eng, ks, last, c["queries"])
        one = (C.c_uint32 * 1)(3)
        lib = eng._lib
        assert lib.s2k_keyset_replace(ks._k, 1, None, key.ctypes.data) == -3 and lib.s2k_keyset_replace(ks._k, 1, one, None) == -3
        assert lib.s2k_keyset_replace_device(ks._k, 1, one, None) == -3 and lib.s2k_keyset_remove(ks._k, 1, None) == -3
        assert lib.s2k_keyset_replace(ks._k, 0, None, None) == 0 and lib.s2k_keyset_remove(ks._k, 0, None) == 0
        ks.replace(np.zeros(0, np.uint32), key[:0])                          # nothing: fine
        with pytest.raises(ValueError):
            ks.replace(np.array([1, 2], np.uint32), key[:1])                 # lengths are checked before the call
        _check_all(eng, S, ks, c, last, layout, cap)
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        ks.close()


# ---- 2. a set without an index ----
@pytest.mark.parametrize("layout", ["KEYSET_JOINT5", "KEYSET_COMB"])
def test_replace_without_an_index(eng, case, layout):
    import secp256k1_voi_amd as S
    c, layout = case, getattr(S, layout)
    states = c["states"][False]
    steps = [st for st in c["steps"] if not st["spare"]]
    ks = eng.keyset_create(states[0]["keys"], layout)
    eng.set_small_batch_max(0)
    eng.set_mid_batch_max(0)
    try:
        for i, step in enumerate(steps[:5]):
            _apply(S, ks, step)
            assert ks.index_info()["slots"] == 0
        _check_all(eng, S, ks, c, states[5], layout, NKEYS, indexed=False)
        ks.index_create()
        _check_all(eng, S, ks, c, states[5], layout, NKEYS)
    finally:
        eng.set_small_batch_max(ROW_DEFAULT)
        eng.set_mid_batch_max(QUAD_DEFAULT)
        ks.close()


# ---- 3. a group's set ----
def test_group_keyset_replace(eng, case):
    import secp256k1_voi_amd as S
    c = case
    states = c["states"][False]
    steps = [st for st in c["steps"] if not st["spare"]]
    grp = S.Group([0])
    try:
        gks = grp.keyset_create(states[0]["keys"], S.KEYSET_JOINT)
        args = (c["kidx_e"], c["dig"], c["r"], c["s"])
        assert np.array_equal(grp.ecdsa_verify_batch_keyset(gks, *args), states[0]["truth_e"])
        for i, step in enumerate(steps):
            slots = np.array(step["slots"], np.uint32)
            if step["op"] == "remove":
                gks.remove(slots)
            else:
                gks.replace(slots, step["keys"])
            assert len(gks) == NKEYS
            assert np.array_equal(grp.ecdsa_verify_batch_keyset(gks, *args), states[i + 1]["truth_e"]), i
        with pytest.raises(S.EngineError):
            gks.replace(np.array([NKEYS], np.uint32), states[0]["keys"][:1])
        with pytest.raises(S.EngineError):
            gks.remove(np.array([4, 4], np.uint32))
        assert np.array_equal(grp.ecdsa_verify_batch_keyset(gks, *args), states[len(steps)]["truth_e"])
        gks.close()
    finally:
        grp.close()
