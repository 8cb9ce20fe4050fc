// sig_prep.h — one signature's scalars prepared by ONE lane: the ECDSA / recovery scalars with their own inversion
// (scalar_prep_one: the preparation waves of small_call.hip's wave-per-signature kernels) and the BIP-340 parse with its challenge
// hash (schnorr_parse*: those waves again, and k_schnorr_prep and the complete-formula BIP-340 kernels of fallback.hip and worklist.hip).
#pragma once
#include "engine_internal.h"
#include "complete_path.h"
#include "sc.h"
#include "sc26.h"
#include "sha256.h"

// What k_scalar_prep (lane_kernels.hip) does for the signatures of a lane,
// for ONE signature, its own inversion, the result in 17 words (u1 | k1 | k2 | flags: the planes' layout): the
// preparation wave of the wave-per-signature kernels (k_verify_row, k_recover_row).  FLAT: the scalar products and the
// inversion are expanded in place (sc26.h), which leaves the kernel without a private segment.
template <bool FLAT = false>
S2K_DEV void scalar_prep_one(size_t i, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig,
                             const uint8_t* __restrict__ recid, uint32_t flags, uint32_t* __restrict__ out17) {
  sc x;
  load_be32(x.v, (recid ? rsig : ssig) + i * 32);      // the value whose inverse is needed
  if (!(sc_is_canonical_raw(x.v) && !sc_is_zero(x))) {   // (rejected below)
    x = sc_zero();
    x.v[0] = 1;
  }
  struct ops {
    static S2K_DEV sc26 mm(const sc26& a, const sc26& b) {
      if constexpr (FLAT) return sc26_montmul(a, b);
      else return sc26_mm(a, b);
    }
    static S2K_DEV sc26 inv_of(const sc26& a) {           // a -> a^-1 * R
      if constexpr (FLAT) return sc26_mont_inv_flat(sc26_to_mont_flat(a));
      else return sc26_mont_inv(sc26_to_mont(a));
    }
  };
  const sc26 s_inv_m = ops::inv_of(sc26_from_sc(x));     // x^-1 * R
  sc r, s;
  uint32_t e_raw[8];
  load_be32(r.v, rsig + i * 32);
  load_be32(s.v, ssig + i * 32);
  load_be32(e_raw, dig + i * 32);
  bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && sc_is_canonical_raw(s.v) && !sc_is_zero(s);
  if (flags & S2K_ECDSA_REJECT_MALLEABLE) ok = ok && !sc_is_gt_half_n(s);
  const sc e = sc_reduce_once(e_raw);
  sc u1, u2;
  uint32_t rid = 0;
  if (recid) {
    rid = recid[i];
    ok = ok && rid < 4 && (!(rid & 2u) || u256_lt(r.v, FE_P_MINUS_N));     // RecoverPoint (point_s11n.go:245-282)
    u1 = sc26_to_sc(ops::mm(sc26_from_sc(sc_neg(e)), s_inv_m));   // -e / r
    u2 = sc26_to_sc(ops::mm(sc26_from_sc(s), s_inv_m));           //  s / r
  } else {
    u1 = sc26_to_sc(ops::mm(sc26_from_sc(e), s_inv_m));
    u2 = sc26_to_sc(ops::mm(sc26_from_sc(r), s_inv_m));
  }
  sc k1, k2;
  bool neg1, neg2;
  sc_split_glv_odd(u2, k1, neg1, k2, neg2);
#pragma unroll
  for (int w = 0; w < 8; ++w) out17[w] = u1.v[w];
#pragma unroll
  for (int w = 0; w < 4; ++w) out17[8 + w] = k1.v[w];
#pragma unroll
  for (int w = 0; w < 4; ++w) out17[12 + w] = k2.v[w];
  out17[16] = (ok ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) | (k1.v[4] ? PF_K1_B128 : 0) | (k2.v[4] ? PF_K2_B128 : 0) |
              ((rid & 3u) << 8);
}

// BIP-340: message i of a batch (offs: variable lengths; else msg_len bytes each)
S2K_DEV void schnorr_msg(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
                         size_t i, const uint8_t*& m, uint32_t& len) {
  if (offs) {
    m = msgs + offs[i];
    len = (uint32_t)(offs[i + 1] - offs[i]);
  } else {
    m = msgs + i * (size_t)msg_len;
    len = msg_len;
  }
}
// parseSchnorrSignature (schnorr.go:420-449): r < p, s < n, e = H(r || P || m) mod n.
// Returns ok; s and e as plain scalars.
// (pk_i: the 32 bytes of item i's x-only key, wherever they live; FLAT: the hash expanded in place, sha256.h)
template <bool FLAT = false>
S2K_DEV bool schnorr_parse_key(size_t i, const uint8_t* __restrict__ pk_i, const uint8_t* __restrict__ sig,
                               const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
                               sc& s_out, sc& e_out) {
  uint32_t r_le[8], pk_le[8];
  load_be32(r_le, sig + i * 64);
  load_be32(s_out.v, sig + i * 64 + 32);
  load_be32(pk_le, pk_i);
  bool ok = fe_is_canonical_raw(r_le) && sc_is_canonical_raw(s_out.v);
  uint32_t r_be[8], pk_be[8], dg[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    r_be[w] = r_le[7 - w];
    pk_be[w] = pk_le[7 - w];
  }
  const uint8_t* m;
  uint32_t len;
  schnorr_msg(msgs, offs, msg_len, i, m, len);
  if constexpr (FLAT) bip340_challenge_flat(dg, r_be, pk_be, m, len);
  else bip340_challenge(dg, r_be, pk_be, m, len);
  uint32_t e_raw[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) e_raw[w] = dg[7 - w];
  e_out = sc_reduce_once(e_raw);
  if (!ok) s_out = sc_zero();
  return ok;
}
S2K_DEV bool schnorr_parse(size_t i, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
                           const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
                           sc& s_out, sc& e_out) {
  return schnorr_parse_key(i, pk + i * 32, sig, msgs, offs, msg_len, s_out, e_out);
}
