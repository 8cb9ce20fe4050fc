// ladder_ecdsa.hip — the ECDSA instantiations of k_verify_fast: the general ladder, the rest of a grouped batch, and the ladders
// over per-key tables, comb tables and key sets; and MODE_POINT, the general ladder without a verdict.
//
// The general ladders stand beside the table ladders on purpose.  The ECDSA ladders over tables (KEYED, COMB, KEYSET*) are the
// same machine code as when engine.hip compiled all eighteen only with a ladder that builds a per-lane table in their unit
// (MODE_POINT alone is enough).  On their own the optimiser leaves their IR different in the verdict - two 32-bit loads it
// otherwise merges, one add-with-carry it otherwise folds - and the kernels come out 2 or 3 instructions longer, registers and
// occupancy unchanged.  Which pass looks beyond the function it works on was not found; tools/kernel_identity.py is the check
// when the grouping changes.  The BIP-340 ladders over tables do not depend on their neighbours (ladder_schnorr.hip).
#include "verify_fast.h"

S2K_LADDER_INSTANCE(MODE_ECDSA)
S2K_LADDER_INSTANCE(MODE_POINT)
S2K_LADDER_INSTANCE(MODE_ECDSA_LEFT)
S2K_LADDER_INSTANCE(MODE_ECDSA_KEYED)
S2K_LADDER_INSTANCE(MODE_ECDSA_COMB)
S2K_LADDER_INSTANCE(MODE_ECDSA_KEYSET)
S2K_LADDER_INSTANCE(MODE_ECDSA_KEYSET_JOINT)
S2K_LADDER_INSTANCE(MODE_ECDSA_KEYSET_JOINT5)
S2K_LADDER_INSTANCE(MODE_ECDSA_KEYSET_JOINT6)
