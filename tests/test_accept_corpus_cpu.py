"""The corpus of tests/accept_corpus.py, checked on the CPU: what tests/test_gpu_accept_rule.py expects of every kernel is what
the C oracle says, every near miss really keeps the parent's R (so only the final comparison can reject it), every claimed bit
position occurs - and a Python model of the accept rule (verify_fast.h: X == r Z^k, then X == (r + n) Z^k under r < p - n) with one
limb masked, one limb left out of the comparison, or the guard dropped changes the verdict of named items."""
import collections
import hashlib

import numpy as np
import pytest

import accept_corpus as A

N, P = A.N, A.P
b32 = A.b32


@pytest.fixture(scope="module")
def corpus(oracle):
    return A.corpus(oracle)


def _int(row):
    return int.from_bytes(bytes(row), "big")


def test_build_time_and_sizes(corpus):
    ec, bip, rec = corpus["ecdsa"], corpus["schnorr"], corpus["recovery"]
    print(f"corpus: {len(ec['cls'])} ECDSA items in {ec['seconds']:.2f} s, {len(bip['cls'])} BIP-340 items in {bip['seconds']:.2f} s, "
          f"{len(rec['cls'])} recovery items")
    assert 900 <= len(ec["cls"]) <= 1300 and 500 <= len(bip["cls"]) <= 700
    assert ec["seconds"] < 10 and bip["seconds"] < 10           # (the C oracle: well under a second each)
    for c, classes in ((ec, A.ECDSA_CLASSES), (bip, A.BIP_CLASSES), (rec, A.REC_CLASSES)):
        count = collections.Counter(c["cls"])
        assert set(count) == set(classes) and all(count[k] > 0 for k in classes), count
    for c in (ec, bip):                                          # valid items: between a tenth and a half
        assert 0.1 * len(c["cls"]) <= int(c["exp"].sum()) <= 0.5 * len(c["cls"])


def test_the_ends_of_the_windows(oracle):
    """x = n and x = p - 3 are on the curve, p - 2 and p - 1 are not (the window of the wrap is [n, p - 3]); n - 2 is, n - 1 is not"""
    for x, on in ((A.X_WRAP_LOW, True), (A.X_WRAP_HIGH, True), (P - 2, False), (P - 1, False), (A.X_TOP, True), (N - 1, False)):
        assert (A.lift_x(oracle, x, 0) is not None) == on, hex(x)
    assert A.X_WRAP_HIGH - N == P - N - 3 and (1 << 128) < P - N


def test_ecdsa_verdicts_are_the_oracles(corpus, oracle):
    ec = corpus["ecdsa"]
    for i, cls in enumerate(ec["cls"]):
        assert bool(ec["exp"][i]) == (cls in A.ECDSA_VALID_CLASSES), (i, cls)
    # (the batch entry point and the single one agree, low s or not)
    for i in range(0, len(ec["cls"]), 7):
        assert oracle.ecdsa_verify_raw(bytes(ec["pub"][i]), bytes(ec["dig"][i]), bytes(ec["r"][i]), bytes(ec["s"][i])) == bool(ec["exp"][i])


def test_ecdsa_keys(corpus, oracle):
    ec = corpus["ecdsa"]
    keys = ec["keys"]
    assert len(keys) == 8 and len({bytes(k) for k in keys}) == 8
    assert keys[0, 63] & 1 == 0 and keys[1, 63] & 1 == 1         # stored with even and with odd Y
    for k, d in enumerate(ec["d"]):
        assert oracle.scalar_base_mult_vartime(b32(d))[1:] == bytes(keys[k])
    per_key = collections.Counter(ec["kidx"].tolist())
    assert all(per_key[k] >= 8 for k in range(8)), per_key       # tables are worth building for every one
    assert np.array_equal(keys[ec["kidx"]], ec["pub"])
    valid_per_key = collections.Counter(ec["kidx"][ec["exp"] == 1].tolist())
    assert all(valid_per_key[k] >= A.FILLERS_PER_KEY for k in range(8))


def test_ecdsa_items_keep_their_point(corpus, oracle):
    """every item: e / s = u1 and r' / s = u2 as recorded, u1 G + u2 Q has the recorded x; every near miss: the u1, u2, key and
    x of its parent - the verifier ends in the parent's R"""
    ec = corpus["ecdsa"]
    seen = set()
    for i, cls in enumerate(ec["cls"]):
        e, r, s, u1, u2 = _int(ec["dig"][i]), _int(ec["r"][i]), _int(ec["s"][i]), ec["u1"][i], ec["u2"][i]
        if 0 < s < N:
            w = pow(s, -1, N)
            assert e * w % N == u1 and r * w % N == u2, (i, cls)
        else:
            assert cls in (A.WRAP_ZERO, A.WRAP_UNREDUCED) and ec["x"][i] == N
        if (u1, u2, int(ec["kidx"][i])) not in seen:
            seen.add((u1, u2, int(ec["kidx"][i])))
            pt = oracle.double_scalar_mult_basepoint_vartime(b32(u1), b32(u2), b"\x04" + bytes(ec["pub"][i]))
            assert pt[0] == 4 and _int(pt[1:33]) == ec["x"][i], (i, cls)
        par = int(ec["parent"][i])
        if cls in A.ECDSA_VALID_CLASSES or cls == A.WRAP_ZERO:
            assert par == -1 and ec["accept"][i] == ec["x"][i] % N
            continue
        assert par >= 0 and ec["cls"][par] in A.ECDSA_VALID_CLASSES + (A.WRAP_ZERO,), (i, cls)
        assert (u1, u2, ec["x"][i], ec["accept"][i]) == (ec["u1"][par], ec["u2"][par], ec["x"][par], ec["accept"][par]), (i, cls)
        assert np.array_equal(ec["pub"][i], ec["pub"][par])


def test_ecdsa_single_bits(corpus):
    """a single-bit item differs from the accepted r in exactly that bit; every bit position claimed occurs, for every R of the
    class that claims all of them"""
    ec = corpus["ecdsa"]
    have = collections.defaultdict(set)
    for i, cls in enumerate(ec["cls"]):
        if cls in A.ECDSA_BIT_CLASSES:
            diff = _int(ec["r"][i]) ^ ec["accept"][i]
            assert diff == 1 << int(ec["bit"][i]) and 0 < _int(ec["r"][i]), (i, cls)
            have[(cls, int(ec["parent"][i]))].add(int(ec["bit"][i]))
        else:
            assert ec["bit"][i] == -1
    per_class = collections.defaultdict(list)
    for (cls, _), bits in have.items():
        per_class[cls].append(bits)
    assert sorted(len(v) for v in per_class.values()) == [1, 1, 3, 3]            # top, small; ordinary and wrapped: three R each
    for cls, want in A.ECDSA_BIT_CLASSES.items():
        full = [b for b in per_class[cls] if b == set(want)]
        assert len(full) >= (2 if cls == A.ORD_BIT else len(per_class[cls])), (cls, [len(b) for b in per_class[cls]])
    # the other near misses are what their names say
    for i, cls in enumerate(ec["cls"]):
        r, x = _int(ec["r"][i]), ec["x"][i]
        if cls == A.ORD_MINUS_N:
            assert (r + N) % 2**256 == x and P - N <= r < N
        elif cls == A.ORD_MINUS_N_MODP:
            assert (r + N) % P == x and P - N <= r < N
        elif cls == A.PLUS_N:
            assert r == x + N and x < P - N
        elif cls == A.WRAP_UNREDUCED:
            assert r == x >= N
        elif cls in (A.WRAP_VALID, A.WRAP_TWIN):
            assert r == x - N and 0 < r < P - N
        elif cls == A.SMALL_VALID:
            assert r == x < 1 << 128
    ends = {ec["x"][i] for i, cls in enumerate(ec["cls"]) if cls in (A.WRAP_VALID, A.WRAP_ZERO)}
    assert {A.X_WRAP_LOW, A.X_WRAP_HIGH} < ends and len(ends) == 3


def test_schnorr_corpus(corpus, oracle):
    bip = corpus["schnorr"]
    keys = bip["keys"]
    assert keys[0, 63] & 1 == 0 and keys[1, 63] & 1 == 1 and np.array_equal(keys[bip["kidx"], :32], bip["pk32"])
    have = collections.defaultdict(set)
    for i, cls in enumerate(bip["cls"]):
        assert bool(bip["exp"][i]) == (cls in A.BIP_VALID_CLASSES), (i, cls)
        par = int(bip["parent"][i])
        if cls in A.BIP_VALID_CLASSES:
            assert par == -1
            continue
        # s G - e P, P the even-y point of the key: the parent's R' for a single-bit item, -R' for the twin
        sig, psig = bytes(bip["sig"][i]), bytes(bip["sig"][par])
        pk_even = A.lift_x(oracle, _int(bip["pk32"][i]), 0)
        pt = oracle.double_scalar_mult_basepoint_vartime(sig[32:], b32(N - bip["e"][i]), pk_even)
        assert bip["cls"][par] == A.BIP_VALID and bip["kidx"][i] == bip["kidx"][par] and np.array_equal(bip["msgs"][i], bip["msgs"][par])
        assert pt[1:33] == psig[:32] and (pt[64] & 1) == (1 if cls == A.BIP_ODD else 0), (i, cls)
        if cls == A.BIP_BIT:
            assert _int(sig[:32]) ^ _int(psig[:32]) == 1 << int(bip["bit"][i])
            have[par].add(int(bip["bit"][i]))
        else:
            assert sig[:32] == psig[:32]
    assert len(have) == 2 and all(b == set(range(256)) for b in have.values())
    assert {int(bip["kidx"][p]) for p in have} == {0, 1}


def test_recovery_corpus(corpus):
    ec, rec = corpus["ecdsa"], corpus["recovery"]
    assert sum(c == A.REC_VALID for c in rec["cls"]) == int(ec["exp"].sum())
    for j, cls in enumerate(rec["cls"]):
        i, v = int(rec["src"][j]), int(rec["rid"][j])
        if cls == A.REC_VALID:
            assert rec["exp_ok"][j] and bytes(rec["exp_pub"][j]) == b"\x04" + bytes(ec["pub"][i])
            assert bool(v & 2) == (ec["x"][i] >= N)
        elif cls == A.REC_BIT1_SET:
            assert not rec["exp_ok"][j] and not rec["exp_pub"][j].any()              # r + n >= p
        else:
            assert ec["x"][i] >= N and bytes(rec["exp_pub"][j, 1:]) != bytes(ec["pub"][i])
    assert any(rec["exp_ok"][j] for j, c in enumerate(rec["cls"]) if c == A.REC_OTHER_PARITY)


# ---- the accept rule as the kernels state it, on 9 limbs of 29 bits (the last one 24), and what a sloppy one would accept ----
W, M29 = 29, (1 << 29) - 1


def _limbs(v):
    return [(v >> (W * j)) & M29 for j in range(8)] + [v >> (W * 8)]


def _mask(v, j):
    return v - (_limbs(v)[j] << (W * j))


def model_ecdsa(r, s, x, z, k, mutation=None):
    """r, s in [1, n), then X == r Z^k or (r < p - n and X == (r + n) Z^k) for X = x Z^k: k = 2 the Jacobian sites, k = 1 the
    homogeneous ones (the row field), k = 0 the affine one.  mutation: ("r", j) limb j of r missing when it becomes a field
    element, ("X", j) / ("rhs", j) limb j of that side of the comparison missing, ("skip", j) limb j not compared,
    ("guard", 256) / ("guard", "p") no r < p - n test, r + n in 256-bit words / in the field."""
    if not (0 < r < N and 0 < s < N):
        return 0
    kind, j = mutation or (None, None)
    zk = pow(z, k, P)
    lhs = x * zk % P
    if kind == "X":
        lhs = _mask(lhs, j)
    cands = [r]
    if r < P - N or kind == "guard":
        cands.append((r + N) % P if j == "p" else (r + N) % 2**256)
    for c in cands:
        if kind == "r":
            c = _mask(c, j)
        rhs = c % P * zk % P
        if kind == "rhs":
            rhs = _mask(rhs, j)
        if kind == "skip":
            if _mask(lhs, j) == _mask(rhs, j):
                return 1
        elif lhs == rhs:
            return 1
    return 0


def _z(i):
    return int.from_bytes(hashlib.sha256(b"accept rule z %d" % i).digest(), "big") % P or 1


def _ecdsa_flips(ec, k, mutation):
    flips = collections.Counter()
    for i, cls in enumerate(ec["cls"]):
        got = model_ecdsa(_int(ec["r"][i]), _int(ec["s"][i]), ec["x"][i], _z(i), k, mutation)
        if got != ec["exp"][i]:
            flips[cls] += 1
    return flips


def test_model_ecdsa_mutations(corpus):
    """The unmutated rule gives the oracle's verdicts at all three sites.  Every mutation flips named items:
      limb j of r, of X or of r Z^k masked (all sites): items of the valid classes turn invalid;
      limb j left out of the affine comparison: single-bit items whose bit lies in limb j turn valid, and nothing else - all
        the ordinary, small and top ones, and those wrapped ones where adding n carries nothing out of the limb; every limb has
        ordinary ones, limbs 0..4 wrapped and small ones too (behind a random Z nothing short of a 2^-29 coincidence shows a
        limb that is not compared: there the valid classes' masks above stand for the site);
      no r < p - n guard: ord_minus_n turns valid where r + n wraps at 2^256, ord_minus_n_modp where it is a field addition."""
    ec = corpus["ecdsa"]
    table = {}
    for k in (2, 1, 0):
        assert not _ecdsa_flips(ec, k, None)
        for j in range(9):
            for kind in ("r", "X", "rhs"):
                f = table[(k, kind, j)] = _ecdsa_flips(ec, k, (kind, j))
                hit_valid = sum(f[c] for c in A.ECDSA_VALID_CLASSES)
                assert hit_valid >= 100 and f[A.FILLER] > 0, (k, kind, j, f)
        assert _ecdsa_flips(ec, k, ("guard", 256)) == {A.ORD_MINUS_N: 3}
        assert _ecdsa_flips(ec, k, ("guard", "p")) == {A.ORD_MINUS_N_MODP: 3}
    for j in range(9):
        f = _ecdsa_flips(ec, 0, ("skip", j))
        lo, hi = W * j, min(W * (j + 1), 256)
        want = collections.Counter(cls for cls, b in zip(ec["cls"], ec["bit"]) if lo <= b < hi)
        assert set(f) <= set(want) and all(f[c] == want[c] for c in want if c != A.WRAP_BIT) and f[A.ORD_BIT] >= 2 * (hi - lo), (j, f, want)
        if j < 5:
            assert want[A.WRAP_BIT] // 2 < f[A.WRAP_BIT] <= want[A.WRAP_BIT] and f[A.SMALL_BIT] == min(hi, 129) - lo, (j, f, want)
    print("flips, Jacobian site:", {key[1:]: dict(v) for key, v in table.items() if key[0] == 2 and key[2] in (0, 8)})


def model_schnorr(r, s, x, y_odd, mutation=None):
    """BIP-340 after the ladder, on the affine point (k_affine_finish; the projective sites compare x Z with r Z as above):
    r < p, s < n, y(R) even, x(R) == r.  mutation: ("skip", j) limb j not compared, ("parity",) the parity not looked at."""
    if r >= P or s >= N:
        return 0
    kind = mutation[0] if mutation else None
    if y_odd and kind != "parity":
        return 0
    return int(_mask(x, mutation[1]) == _mask(r, mutation[1])) if kind == "skip" else int(x == r)


def test_model_schnorr_mutations(corpus):
    bip = corpus["schnorr"]

    def flips(mutation):
        out = collections.Counter()
        for i, cls in enumerate(bip["cls"]):
            par = int(bip["parent"][i])
            x = _int(bip["sig"][par if par >= 0 else i][:32])                # x(R): the parent's r (test_schnorr_corpus)
            got = model_schnorr(_int(bip["sig"][i][:32]), _int(bip["sig"][i][32:]), x, cls == A.BIP_ODD, mutation)
            if got != bip["exp"][i]:
                out[cls] += 1
        return out

    assert not flips(None)
    assert flips(("parity",)) == {A.BIP_ODD: 2}
    for j in range(9):
        assert flips(("skip", j)) == {A.BIP_BIT: 2 * (min(W * (j + 1), 256) - W * j)}, j
