"""Stage-timing records of the key-set device forms (s2k_ctx_profile / s2k_ctx_profile_read_stages): which forms leave a record
per call and which leave none, on the lane-per-signature path and on the wave-per-signature (row) path.

By-index ECDSA (s2k_ecdsa_verify_batch_keyset_device) records every call, row and lane - bench.py reads `fast_ms` and `calls`
from it; the two by-key forms record every call; by-index BIP-340 (s2k_schnorr_verify_batch_keyset_device) records none on
either path.  Every group's verdicts are the oracle's.

257 signatures (a full workgroup and one lane) over a set of 37 keys; the by-key batches also carry keys the set does not hold.
The builders are shared with test_gpu_keyset_refused_then_good.py."""
import os

import numpy as np
import pytest

import test_gpu_schnorr_bykey as SB
import test_gpu_schnorr_comb as SC

pytestmark = pytest.mark.gpu
NSIG, NKEYS, NPOOL = 257, 37, 45
KS_ROW_DEFAULT = 2048


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def ecdsa_case(eng, oracle, seed):
    """320 signatures of 45 keys (signature i under key i mod 45), every seventh damaged in r, s or the digest; the set holds
    keys 0 .. 36.  `index`: the first 257 signatures under a key of the set, named by index; `bykey`: the first 257 of all,
    an eighth of them under keys the set does not hold.  Expected verdicts: the oracle's."""
    from secp256k1_voi_amd.synth import synth_batch
    pub, dig, r, s = (np.array(a) for a in synth_batch(eng, 320, NPOOL, seed=seed))
    key = np.arange(320) % NPOOL
    keys = np.ascontiguousarray(pub[:NKEYS])
    assert len(np.unique(pub[:NPOOL], axis=0)) == NPOOL
    for j, i in enumerate(range(3, 320, 7)):
        (r, s, dig)[j % 3][i, 5 + j % 20] ^= 1 << (j % 8)
    rows = np.nonzero(key < NKEYS)[0][:NSIG]
    assert rows.size == NSIG
    out = {"keys": keys}
    for name, sel in (("index", rows), ("bykey", np.arange(NSIG))):
        a = [np.ascontiguousarray(x[sel]) for x in (pub, dig, r, s)]
        exp = oracle.ecdsa_verify_batch(*a, nthreads=os.cpu_count() or 1)
        assert 0.7 * NSIG < int(exp.sum()) < NSIG
        out[name] = dict(kidx=key[sel].astype(np.uint32), pub=a[0], dig=a[1], r=a[2], s=a[3], exp=exp)
    assert (key[:NSIG] >= NKEYS).sum() >= NSIG // 8 - 2 and out["bykey"]["exp"][key[:NSIG] >= NKEYS].any()
    return out


def schnorr_case(eng, oracle, seed):
    """the same for BIP-340: x-only keys, 32-byte messages; the set holds the keys 0 .. 36 as X || Y, every other one with odd Y"""
    from secp256k1_voi_amd.synth import synth_schnorr_batch
    pk, msgs, sig = (np.array(a) for a in synth_schnorr_batch(eng, 320, NPOOL, seed=seed))
    key = np.arange(320) % NPOOL
    assert len({bytes(x) for x in pk[:NPOOL]}) == NPOOL
    keys = SB._lifted(pk[:NKEYS])
    for j, i in enumerate(range(3, 320, 7)):
        if j % 3 < 2:
            sig[i, 32 * (j % 3) + 5 + j % 20] ^= 1 << (j % 8)
        else:
            msgs[i, j % 32] ^= 1 << (j % 8)
    rows = np.nonzero(key < NKEYS)[0][:NSIG]
    out = {"keys": keys}
    for name, sel in (("index", rows), ("bykey", np.arange(NSIG))):
        a = [np.ascontiguousarray(x[sel]) for x in (pk, msgs, sig)]
        exp = SC.expected(oracle, a[0], [bytes(m) for m in a[1]], a[2])
        assert 0.7 * NSIG < int(exp.sum()) < NSIG
        out[name] = dict(kidx=key[sel].astype(np.uint32), pk=a[0], msgs=a[1], sig=a[2], exp=exp)
    assert out["bykey"]["exp"][key[:NSIG] >= NKEYS].any()
    return out


@pytest.fixture(scope="module")
def cases(eng, oracle):
    return ecdsa_case(eng, oracle, 2101), schnorr_case(eng, oracle, 2102)


def test_stage_records_per_form(eng, cases):
    import torch
    import secp256k1_voi_amd as S
    ec, sc = cases
    dev = torch.device("cuda", 0)
    up = lambda *arrs: [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrs]
    ks_e = eng.keyset_create(ec["keys"], S.KEYSET_JOINT5)
    ks_s = eng.keyset_create(sc["keys"], S.KEYSET_JOINT5)
    try:
        ks_e.index_create()
        ks_s.index_create()
        ei, eb, si, sb = ec["index"], ec["bykey"], sc["index"], sc["bykey"]
        t_ei = up(ei["kidx"].view(np.int32), ei["dig"], ei["r"], ei["s"])
        t_eb = up(eb["pub"], eb["dig"], eb["r"], eb["s"])
        t_si = up(si["kidx"].view(np.int32), si["msgs"], si["sig"])
        t_sb = up(sb["pk"], sb["msgs"], sb["sig"])
        p = lambda ts: [t.data_ptr() for t in ts]

        def ecdsa_index(out):
            eng.ecdsa_verify_batch_keyset_device(ks_e, NSIG, *p(t_ei), out.data_ptr())

        def ecdsa_bykey(out):
            eng.ecdsa_verify_batch_bykey_device(ks_e, NSIG, *p(t_eb), out.data_ptr())

        def schnorr_index(out):
            eng.schnorr_verify_batch_keyset_device(ks_s, NSIG, t_si[0].data_ptr(), t_si[1].data_ptr(), 32, t_si[2].data_ptr(), out.data_ptr())

        def schnorr_bykey(out):
            eng.schnorr_verify_batch_bykey_device(ks_s, NSIG, t_sb[0].data_ptr(), t_sb[1].data_ptr(), 32, t_sb[2].data_ptr(), out.data_ptr())

        # (name, call, keyset_small_batch_max, expected ladder, expected records, expected verdicts)
        LANE, ROW = S.KEYSET_LADDER_LANE, S.KEYSET_LADDER_ROW
        groups = [("ecdsa by index, lane", ecdsa_index, 0, LANE, 3, ei["exp"]),
                  ("ecdsa by index, row", ecdsa_index, KS_ROW_DEFAULT, ROW, 3, ei["exp"]),
                  ("ecdsa by key", ecdsa_bykey, 0, LANE, 3, eb["exp"]),
                  ("bip340 by key", schnorr_bykey, 0, LANE, 3, sb["exp"]),
                  ("bip340 by index, lane", schnorr_index, 0, LANE, 0, si["exp"]),
                  ("bip340 by index, row", schnorr_index, KS_ROW_DEFAULT, ROW, 0, si["exp"])]
        eng.set_small_batch_max(0)          # (the by-key forms would be the plain call at this size)
        eng.set_mid_batch_max(0)
        eng.profile(True)
        try:
            for name, call, row_max, ladder, records, exp in groups:
                eng.set_keyset_small_batch_max(row_max)
                outs = [torch.full((NSIG,), 7, dtype=torch.uint8, device=dev) for _ in range(3)]
                for out in outs:
                    call(out)
                    assert eng.last_keyset_ladder() == ladder, name
                st = eng.profile_read_stages()
                assert st["calls"] == records, (name, st["calls"])
                for out in outs:
                    got = out.cpu().numpy()
                    assert np.array_equal(got, exp), (name, np.nonzero(got != exp)[0][:10])
        finally:
            eng.profile(False)
            eng.set_keyset_small_batch_max(KS_ROW_DEFAULT)
            eng.set_small_batch_max(SB.ROW_DEFAULT)
            eng.set_mid_batch_max(SB.QUAD_DEFAULT)
    finally:
        ks_e.close()
        ks_s.close()
