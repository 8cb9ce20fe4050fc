// ladder_schnorr.hip — the BIP-340 instantiations of k_verify_fast that take their points from tables: per-key tables, comb
// tables and key sets.  (MODE_SCHNORR and MODE_SCHNORR_LEFT lift their keys themselves and are instantiated in fallback.hip.)
#include "verify_fast.h"

S2K_LADDER_INSTANCE(MODE_SCHNORR_KEYED)
S2K_LADDER_INSTANCE(MODE_SCHNORR_COMB)
S2K_LADDER_INSTANCE(MODE_SCHNORR_KEYSET)
S2K_LADDER_INSTANCE(MODE_SCHNORR_KEYSET_JOINT)
S2K_LADDER_INSTANCE(MODE_SCHNORR_KEYSET_JOINT5)
S2K_LADDER_INSTANCE(MODE_SCHNORR_KEYSET_JOINT6)
