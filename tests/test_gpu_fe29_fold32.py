"""The 9x29 products with 32-bit upper digits on the device: every generated form through the hot-path hook
(s2k_fp_op_batch_ex: S2K_HP_MUL, _SQR, _MUL_PLUS, _SQR_PLUS, _MUL_ADD_MUL, _MUL_ADD_SQR) on 4096 lanes of operands in
lazy form, against Python integers mod p, and two 4096-signature verification calls (256 keys x 16 with per-key tables;
the same with the grouping off) with damaged subsets against the oracle: the smallest calls that reach k_key_chain,
k_key_finish, k_generator_part and both lane ladders (the wave- and quad-per-signature ladders are switched off).

The lanes hold 0, 1, p - 1, p and 2^256 - 1 against each other (p, and 2p through the lazy codes, are the lazy forms of
0; 2^256 - 1 has every limb at its mask, plus the multiples of p the code adds), carry-path limb patterns and random
values.  The CPU model of the generated header (tests/fe29_fold32_model.py) runs on the first lanes of every case and
must see, for every upper column 9..16, a lane whose digit has bits 29..31 all set: digits the 29-bit split never made.
"""
import os
import random

import numpy as np
import pytest

import fe29_fold32_model as F
import pyref as R

pytestmark = pytest.mark.gpu
P = R.P
b32 = R.b32
LANES = 4096
MODELLED = 384          # lanes per case that also run through the CPU model (coverage of the wide digits)
SPECIAL = [0, 1, P - 1, P, 2**256 - 1]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    e.set_small_batch_max(0)       # 4096 signatures on the lane ladders, not one wave or quad per signature
    e.set_mid_batch_max(0)
    return e


def units(code):
    return 1 + (code & 3) + (1 if code & 4 else 0)


def lazy(*codes):
    v = 0
    for j, c in enumerate(codes):
        v |= c << (4 * j)
    return v


def structured(rnd, count):
    pats = [0, 1, 2**29 - 1, 2**28, 2**28 - 1, 2**29 - 2, 0x1FFFFC2F, 0x1FFFFFF7]
    top = [0, 1, 2**24 - 1, 2**24 - 2, 2**23, 2**23 - 1]
    return [sum(rnd.choice(pats) << (29 * i) for i in range(8)) | rnd.choice(top) << 232 for _ in range(count)]


def operands(seed, n_ops):
    """n_ops lists of LANES values: the specials against each other in the first two, then random (the modelled lanes),
    limb patterns, values next to p and 2^256, random"""
    rnd = random.Random(seed)
    front = len(SPECIAL) ** 2
    out = []
    for j in range(n_ops):
        if j == 0:
            head = [s for s in SPECIAL for _ in SPECIAL]
        elif j == 1:
            head = [t for _ in SPECIAL for t in SPECIAL]
        else:
            head = [rnd.choice(SPECIAL) for _ in range(front)]
        body = [rnd.randrange(2**256) for _ in range(MODELLED)] + structured(rnd, 1500) + \
            [rnd.randrange(P - 2**40, 2**256) for _ in range(300)]
        body += [rnd.randrange(2**256) for _ in range(LANES - front - len(body))]
        tail = body[MODELLED:]
        rnd.shuffle(tail)
        out.append(head + body[:MODELLED] + tail)
        assert len(out[-1]) == LANES
    return out


# op name -> (generated function, lazy-code cases within the unit budget of fe29.h: at most 7 units, as test_gpu_hotpath.py keeps it)
CASES = {
    "HP_MUL": ("fe29_mul", [(0, 0), (2, 1), (1, 2), (7, 0), (0, 6)]),
    "HP_SQR": ("fe29_sqr", [(0,), (1,), (4,)]),
    "HP_MUL_PLUS": ("fe29_mul_plus", [(0, 0, 0), (2, 1, 0), (4, 4, 2), (0, 5, 1)]),
    "HP_SQR_PLUS": ("fe29_sqr_plus", [(0, 0), (1, 2), (4, 2), (0, 6)]),
    "HP_MUL_ADD_MUL": ("fe29_mul_add_mul", [(0, 0, 0, 0), (2, 1, 0, 0), (1, 1, 1, 0), (0, 0, 4, 1), (1, 0, 0, 7)]),
    "HP_MUL_ADD_SQR": ("fe29_mul_add_sqr", [(0, 0, 0), (1, 1, 0), (2, 1, 0), (0, 2, 1)]),
}


def budget(fn, codes):
    u = [units(c) for c in codes]
    return {"fe29_mul": lambda: u[0] * u[1], "fe29_sqr": lambda: u[0] ** 2, "fe29_mul_plus": lambda: u[0] * u[1] + u[2],
            "fe29_sqr_plus": lambda: u[0] ** 2 + u[1], "fe29_mul_add_mul": lambda: u[0] * u[1] + u[2] * u[3],
            "fe29_mul_add_sqr": lambda: u[0] * u[1] + u[2] ** 2}[fn]()


@pytest.mark.parametrize("op,codes", [(op, c) for op, (_, cases) in CASES.items() for c in cases])
def test_products_on_lazy_operands(eng, op, codes):
    import secp256k1_voi_amd as S
    fn = CASES[op][0]
    names, exact = F.FORMS[fn]
    assert budget(fn, codes) <= 7
    vals = operands(sum(codes) * 97 + len(op), len(names))
    want = [exact(*xs) % P for xs in zip(*vals)]
    # the model on the lanes behind the specials: the same limbs the device builds, and the wide digits are there
    funcs = F.functions()
    first = len(SPECIAL) ** 2
    seen = [0] * 8
    for i in list(range(first)) + list(range(first, first + MODELLED)):
        digits = []
        limbs = {nm: F.lazy_form(v[i], c) for nm, v, c in zip(names, vals, codes)}
        r = F.run(funcs[fn], limbs, digits=digits)
        F.check_result(r, want[i])
        for k, u in enumerate(digits):
            seen[k] += (u >> 29) == 7
    assert all(seen), seen
    out, _, _ = eng.fp_op_batch_ex(getattr(S, op), [[b32(x) for x in v] for v in vals], lazy(*codes))
    got = [int.from_bytes(bytes(x), "big") for x in np.asarray(out)]
    bad = [i for i in range(LANES) if got[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
    # canonical output: S2K_HP_NORMALIZE leaves it as it is
    norm, _, flag = eng.fp_op_batch_ex(S.HP_NORMALIZE, [out], 0)
    assert np.array_equal(norm, out) and [int(f) for f in flag] == [int(w == 0) for w in want]


def _damage(pub, dig, r, s, seed):
    """a seeded quarter of the signatures damaged: a flipped bit in r, s or the digest, r = 0, s = 0, another key"""
    n = len(pub)
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 24, size=n)
    for k, a in ((0, r), (1, s), (2, dig)):
        i = np.nonzero(kind == k)[0]
        a[i, rng.integers(0, 32, size=i.size)] ^= (1 << rng.integers(0, 8, size=i.size)).astype(np.uint8)
    r[kind == 3] = 0
    s[kind == 4] = 0
    i = np.nonzero(kind == 5)[0]
    pub[i] = pub[(i + 1) % n]
    return kind


def _device_run(eng, pub, dig, r, s):
    import torch
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pub, dig, r, s)]
    out = torch.empty(len(pub), dtype=torch.uint8, device=dev)
    eng.ecdsa_verify_batch_device(len(pub), *(x.data_ptr() for x in t), out.data_ptr())
    torch.cuda.synchronize()
    return out.cpu().numpy(), eng.key_grouping_stats()


@pytest.fixture(scope="module")
def batch(eng, oracle):
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = (np.array(x) for x in synth_batch(eng, LANES, 256, seed=1032))
    kind = _damage(pub, dig, r, s, 2932)
    exp = oracle.ecdsa_verify_batch(pub, dig, r, s, nthreads=min(16, os.cpu_count() or 1))
    assert 0.6 * LANES < int(exp.sum()) < LANES and not exp[(kind == 3) | (kind == 4)].any()
    return pub, dig, r, s, exp


def test_keyed_call_matches_oracle(eng, batch):
    """256 keys x 16 signatures: per-key tables (k_key_chain, k_key_finish), k_generator_part, the keyed lane ladder"""
    import secp256k1_voi_amd as S
    pub, dig, r, s, exp = batch
    eng.set_key_grouping(S.KEYS_AUTO)
    got, st = _device_run(eng, pub, dig, r, s)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    assert st["keyed"] + st["general"] == LANES and st["keyed"] > LANES // 2 and st["tables"] >= 128, st


def test_general_call_matches_oracle(eng, batch):
    """the same signatures with the grouping off: the general lane ladder for every one of them"""
    import secp256k1_voi_amd as S
    pub, dig, r, s, exp = batch
    eng.set_key_grouping(S.KEYS_OFF)
    try:
        got, st = _device_run(eng, pub, dig, r, s)
    finally:
        eng.set_key_grouping(S.KEYS_AUTO)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0][:10]
    assert st["keyed"] == 0 and st["tables"] == 0, st
