"""A key-set call that is refused leaves nothing behind: the next call on the same context, of another batch, gives the
oracle's verdicts and s2k_wait_all returns S2K_OK.  The four synchronous host forms over a key set and their four _submit
forms, through the C entry points.

Where the refusal happens (keyset.hip; S2K_ERR_ARG each time):
  s2k_ecdsa_verify_batch_keyset                 S2K_ECDSA_FORCE_COMPLETE is checked only INSIDE the device form: the inputs are
                                                staged and their copies enqueued when the call is refused
  s2k_schnorr_verify_batch_keyset               a non-zero flag is checked only INSIDE the device form, as above
  s2k_ecdsa_verify_batch_keyset_bykey           before staging (bykey_check)
  s2k_schnorr_verify_batch_keyset_bykey         before staging (schnorr_bykey_args)
  the four _submit forms                        before a ticket slot is taken, so before staging
A refusal after the copies were enqueued must drain the context: the buffers those copies fill are the next call's.

257 signatures over a set of 37 keys: valid and damaged signatures, and for the forms by key bytes keys the set does not hold
(test_gpu_keyset_marks.py builds them).  The refused call carries the batch in reverse order, the good call the batch itself."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_keyset_marks as KM
import test_gpu_schnorr_bykey as SB

pytestmark = pytest.mark.gpu
NSIG = KM.NSIG
S2K_OK, S2K_ERR_ARG = 0, -3


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    import secp256k1_voi_amd as S
    e = S.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(eng, oracle):
    return KM.ecdsa_case(eng, oracle, 2111), KM.schnorr_case(eng, oracle, 2112)


def _args(case, first):
    """(good, reversed) argument arrays of a case: `first` names the leading array (kidx, pub or pk)"""
    names = [first] + [k for k in ("dig", "r", "s", "msgs", "sig") if k in case]
    good = [np.ascontiguousarray(case[k]) for k in names]
    return good, [np.ascontiguousarray(a[::-1]) for a in good]


FORMS = ["ecdsa_keyset", "ecdsa_bykey", "schnorr_keyset", "schnorr_bykey"]


@pytest.mark.parametrize("submit", [False, True], ids=["sync", "submit"])
@pytest.mark.parametrize("form", FORMS)
def test_refused_then_good(eng, cases, form, submit):
    import secp256k1_voi_amd as S
    ec, sc = cases
    ecdsa, bykey = form.startswith("ecdsa"), form.endswith("bykey")
    case = (ec if ecdsa else sc)["bykey" if bykey else "index"]
    good, rev = _args(case, ("pub" if ecdsa else "pk") if bykey else "kidx")
    fn = getattr(eng._lib, {"ecdsa_keyset": "s2k_ecdsa_verify_batch_keyset", "ecdsa_bykey": "s2k_ecdsa_verify_batch_keyset_bykey",
                            "schnorr_keyset": "s2k_schnorr_verify_batch_keyset", "schnorr_bykey": "s2k_schnorr_verify_batch_keyset_bykey"}[form]
                 + ("_submit" if submit else ""))
    bad_flag = S.FORCE_COMPLETE if ecdsa else S.REJECT_MALLEABLE
    ks = eng.keyset_create((ec if ecdsa else sc)["keys"], S.KEYSET_JOINT5)
    eng.set_small_batch_max(0)              # (the forms by key bytes would be the plain call at this size)
    eng.set_mid_batch_max(0)
    eng.set_keyset_small_batch_max(0)       # the lane-per-signature path
    try:
        ks.index_create()

        def call(a, flags, out):
            p = [x.ctypes.data for x in a]
            tk = C.c_uint64(0)
            tail = (C.byref(tk),) if submit else ()
            if ecdsa:
                rc = fn(eng._h, ks._k, NSIG, p[0], p[1], p[2], p[3], flags, out.ctypes.data, *tail)
            else:
                rc = fn(eng._h, ks._k, NSIG, p[0], p[1], None, 32, p[2], flags, out.ctypes.data, *tail)
            return rc, tk.value

        out_bad = np.full(NSIG, 7, np.uint8)
        rc, tk = call(rev, bad_flag, out_bad)
        assert rc == S2K_ERR_ARG and tk == 0, (rc, tk)
        out = np.full(NSIG, 7, np.uint8)
        rc, tk = call(good, 0, out)
        assert rc == S2K_OK, (rc, eng._lib.s2k_last_error(eng._h))
        if submit:
            assert tk != 0 and eng._lib.s2k_wait(eng._h, tk) == S2K_OK
        assert np.array_equal(out, case["exp"]), np.nonzero(out != case["exp"])[0][:10]
        assert 0 < int(out.sum()) < NSIG
        assert eng.last_keyset_ladder() == S.KEYSET_LADDER_LANE or submit      # (a ticket runs on a child context)
        assert eng._lib.s2k_wait_all(eng._h) == S2K_OK
    finally:
        eng.set_keyset_small_batch_max(KM.KS_ROW_DEFAULT)
        eng.set_small_batch_max(SB.ROW_DEFAULT)
        eng.set_mid_batch_max(SB.QUAD_DEFAULT)
        ks.close()
