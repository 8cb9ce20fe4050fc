"""The boundary of the comb sets' small-call ladder without a GPU: the setter, its group form, the third ladder code and the
test operation are in the header, in the built library and in the binding, with the values the header gives them."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("s2k_ctx_set_keyset_comb_small_batch_max", "s2k_group_set_keyset_comb_small_batch_max")


def header():
    with open(os.path.join(ROOT, "include", "secp256k1_voi_amd.h")) as f:
        return f.read()


def test_header_declares_them():
    src = header()
    assert re.search(r"int s2k_ctx_set_keyset_comb_small_batch_max\(s2k_ctx \*ctx, uint32_t max_n\);", src)
    assert re.search(r"int s2k_group_set_keyset_comb_small_batch_max\(s2k_group \*g, uint32_t max_n\);", src)
    codes = dict(re.findall(r"#define (S2K_KEYSET_LADDER_[A-Z_]+) (\d+)", src))
    assert codes == {"S2K_KEYSET_LADDER_LANE": "0", "S2K_KEYSET_LADDER_ROW": "1", "S2K_KEYSET_LADDER_ROW_COMB": "2"}
    # the operation is appended: the last enumerator, right behind S2K_HP_JADD_PAIR
    body = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"S2K_HP_JADD_PAIR\s*,\s*S2K_HP_PT29R_COMB_STEP\s*\}", body)


def test_binding_and_library_have_them():
    import secp256k1_voi_amd as S
    assert (S.KEYSET_LADDER_LANE, S.KEYSET_LADDER_ROW, S.KEYSET_LADDER_ROW_COMB) == (0, 1, 2)
    assert S.HP_PT29R_COMB_STEP == S.HP_JADD_PAIR + 1 == S.HP_PT29R_ADD_B3 + 2
    assert all(n in S.EXPORTED_SYMBOLS for n in NEW)
    assert callable(S.Engine.set_keyset_comb_small_batch_max) and callable(S.Group.set_keyset_comb_small_batch_max)
    S.build()
    lib = S.load_library()
    for n in NEW:
        assert hasattr(lib, n), n
    # argument checks run without a device
    assert lib.s2k_ctx_set_keyset_comb_small_batch_max(None, 2048) == -3          # S2K_ERR_ARG
    assert lib.s2k_group_set_keyset_comb_small_batch_max(None, 2048) == -3
