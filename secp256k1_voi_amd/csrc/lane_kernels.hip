// lane_kernels.hip — the kernels around the lane-per-signature ladders: scalar preparation (k_scalar_prep, k_schnorr_prep,
// k_hot_prep), the generator part of the grouped flows (k_generator_part) and the affine epilogue (k_affine_finish), with
// their launchers, and launch_ladder, which launches the ladders themselves: k_verify_fast<MODE> (verify_fast.h, instantiated
// in the ladder_*.hip units) and k_verify_comb (comb_ladder.hip).  The call flows that use them: engine.hip, keyset.hip.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "engine_internal.h"
#include "fe.h"
#include "fe29_inv.h"
#include "jacobian29.h"
#include "xyzz29.h"
#include "lane_tables.h"
#include "pt29.h"
#include "complete_path.h"
#include "point.h"
#include "sc.h"
#include "sc26.h"
#include "sig_prep.h"

using namespace s2k;

// ---------------------------------------------------------------------------------------
// Fast path, kernel 1: scalar preparation with batched inversion.
// Each thread owns PREP_M signatures (i = t, t+T, t+2T, ...): one inversion mod n (safegcd
// division steps, modinv30.h; the reference's Scalar.Invert is a Fermat chain,
// scalar_invert.go:11) is shared by PREP_M signatures through Montgomery's trick, 3 extra
// multiplications each, instead of one inversion per signature as in verify (ecdsa.go:428).
// PREP_M trades inversions against waves: measured at 2^20 (tools/ab_prep.sh) 2: 413, 3: 340,
// 4: 285, 6: 276, 8: 299, 16: 356, 32: 450 us (with the Fermat chain: 16: 466 us).
// Out per signature (word-major, coalesced):
//   u1 (8 words), |k1|, |k2| (4 words each; u2 = +-k1 +- k2*lambda), flag word.
// ---------------------------------------------------------------------------------------
constexpr int PREP_M = S2K_PREP_M;   // (S2K_PREP_M and PREP_WORDS: engine_internal.h)
// (the flag word's bits, PF_*: engine_internal.h)

S2K_DEV void ws_store_sc26(uint32_t* __restrict__ base, size_t stride, size_t i, const sc26& v) {
#pragma unroll
  for (int w = 0; w < 10; ++w) base[(size_t)w * stride + i] = v.n[w];
}
S2K_DEV sc26 ws_load_sc26(const uint32_t* __restrict__ base, size_t stride, size_t i) {
  sc26 r;
#pragma unroll
  for (int w = 0; w < 10; ++w) r.n[w] = base[(size_t)w * stride + i];
  return r;
}

// recid != nullptr selects public-key recovery (RecoverPublicKey, ecdsa.go:244-282): the shared
// inversion is of r instead of s, and u1 = -e/r, u2 = s/r.
__global__ void __launch_bounds__(64)
k_scalar_prep(uint32_t n, uint32_t T, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig,
              const uint8_t* __restrict__ ssig, const uint8_t* __restrict__ recid, uint32_t flags,
              uint32_t* __restrict__ prep, uint32_t* __restrict__ pref, uint32_t* __restrict__ smont, size_t stride) {
  uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  // products run on the lazy 10x26 Montgomery form (sc26.h); pref/smont are 10-word planes
  sc26 one_m = sc26_from_limbs(SC26_ONE_M);
  sc26 acc = one_m;
#pragma unroll 1
  for (int j = 0; j < PREP_M; ++j) {
    size_t i = (size_t)t + (size_t)j * T;
    if (i >= n) break;
    sc s;
    load_be32(s.v, (recid ? rsig : ssig) + i * 32);   // the value whose inverse is needed
    bool ok_s = sc_is_canonical_raw(s.v) && !sc_is_zero(s);
    if (!ok_s) {   // keep the shared product invertible; the signature is rejected below
      s = sc_zero();
      s.v[0] = 1;
    }
    sc26 sm = sc26_to_mont(sc26_from_sc(s));
    ws_store_sc26(smont, stride, i, sm);
    acc = sc26_mm(acc, sm);
    ws_store_sc26(pref, stride, i, acc);
  }
  sc26 inv = sc26_mont_inv(acc);
#pragma unroll 1
  for (int j = PREP_M - 1; j >= 0; --j) {
    size_t i = (size_t)t + (size_t)j * T;
    if (i >= n) continue;
    sc26 sm = ws_load_sc26(smont, stride, i);
    sc26 prev = j > 0 ? ws_load_sc26(pref, stride, i - T) : one_m;
    sc26 s_inv_m = sc26_mm(inv, prev);             // s_i^-1 * R
    inv = sc26_mm(inv, sm);
    sc r, s;
    uint32_t e_raw[8];
    load_be32(r.v, rsig + i * 32);
    load_be32(s.v, ssig + i * 32);
    load_be32(e_raw, dig + i * 32);
    bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && sc_is_canonical_raw(s.v) && !sc_is_zero(s);
    if (flags & S2K_ECDSA_REJECT_MALLEABLE) ok = ok && !sc_is_gt_half_n(s);
    sc e = sc_reduce_once(e_raw);
    sc u1, u2;
    uint32_t rid = 0;
    if (recid) {
      rid = recid[i];
      // RecoverPoint (point_s11n.go:245-282): id in [0,3]; bit 1 means x = r + n, which must stay < p
      ok = ok && rid < 4 && (!(rid & 2u) || u256_lt(r.v, FE_P_MINUS_N));
      u1 = sc26_to_sc(sc26_mm(sc26_from_sc(sc_neg(e)), s_inv_m));   // -e / r
      u2 = sc26_to_sc(sc26_mm(sc26_from_sc(s), s_inv_m));           //  s / r
    } else {
      u1 = sc26_to_sc(sc26_mm(sc26_from_sc(e), s_inv_m));
      u2 = sc26_to_sc(sc26_mm(sc26_from_sc(r), s_inv_m));
    }
    sc k1, k2;
    bool neg1, neg2;
    sc_split_glv_odd(u2, k1, neg1, k2, neg2);          // both halves odd, < 2^129
    uint32_t f = (ok ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) |
                 (k1.v[4] ? PF_K1_B128 : 0) | (k2.v[4] ? PF_K2_B128 : 0) | ((rid & 3u) << 8);
#pragma unroll
    for (int w = 0; w < 8; ++w) prep[(size_t)w * stride + i] = u1.v[w];
#pragma unroll
    for (int w = 0; w < 4; ++w) prep[(size_t)(8 + w) * stride + i] = k1.v[w];
#pragma unroll
    for (int w = 0; w < 4; ++w) prep[(size_t)(12 + w) * stride + i] = k2.v[w];
    prep[(size_t)16 * stride + i] = f;
  }
}

// Lanes of k_scalar_prep for n signatures: PREP_M signatures share a lane's inversion where that saves instructions that
// matter (2^20: a third of the kernel), but a call that cannot fill the chip anyway is better off with the latency of fewer
// signatures per lane - up to 2^16 lanes (a wave on every SIMD) are used before signatures start to share one (94 us for six in
// a row, 55 for one).
__attribute__((visibility("hidden"))) uint32_t prep_lanes(size_t n) {
  const size_t shared = (n + PREP_M - 1) / PREP_M, wide = n < ((size_t)1 << 16) ? n : ((size_t)1 << 16);
  return (uint32_t)(shared > wide ? shared : wide);
}

// ---------------------------------------------------------------------------------------
// Grouped flow only: the generator part u1*G of every signature, on its own.  It needs nothing but
// the prepared u1, so it runs on the second stream, after the scalar preparation and beside the
// grouping and per-key table kernels (which are latency or memory bound and leave the multipliers
// idle); the ladders then finish with one Jacobian + Jacobian addition instead of GT_WINDOWS mixed ones.
// Out: (X, Y, Z) in three "fin"-format elements per SIGNATURE (gp planes).  A degenerate addition
// on the way (or u1 = 0) leaves Z = 0, which the ladder's final addition passes on to the worklist.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_generator_part(uint32_t first, uint32_t n, const uint32_t* __restrict__ prep, gt_view gt,
                 uint32_t* __restrict__ gp, size_t stride) {
  size_t idx = (size_t)first + (size_t)blockIdx.x * 256 + threadIdx.x;   // signatures [first, n)
  if (idx >= n) return;
  uint32_t u[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) u[w] = prep[(size_t)w * stride + idx];
  apt g = gt_load(gt, 0, gt_next_digit(u, gt.bits));
  const fe29 ax = fe29_from_words(g.x.v), ay = fe29_from_words(g.y.v);
  xyzz29 xa = xyzz29_from_affine(ax, ay);                                            // XYZZ additions, as in the keyed ladder
  g = gt_load(gt, 1, gt_next_digit(u, gt.bits));
  if (gt.windows > 1) {   // the first addition: both points affine
    const fe29 gx = fe29_from_words(g.x.v), gy = fe29_from_words(g.y.v);
    if (gt.windows > 2) g = gt_load(gt, 2, gt_next_digit(u, gt.bits));
    xa = xyzz29_add_affine_first(ax, ay, gx, gy);
  }
#pragma unroll 1
  for (uint32_t w = 2; w < gt.windows; ++w) {
    const fe29 gx = fe29_from_words(g.x.v), gy = fe29_from_words(g.y.v);
    if (w + 1 < gt.windows) g = gt_load(gt, w + 1, gt_next_digit(u, gt.bits));   // in flight during this addition
    xa = xyzz29_add_affine(xa, gx, gy);
  }
  // (two entries in flight instead of one halve the kernel's waiting - SQ_WAIT_ANY 87 M -> 46 M wave cycles - and change
  // neither its duration nor the step's: three waves per SIMD cover it; profiles/r06_wait_shares.txt)
  const jpt29 acc = xyzz29_to_jacobian(xa);
  fq_store(gp, stride, idx, 0, acc.x);
  fq_store(gp, stride, idx, 1, acc.y);
  fq_store(gp, stride, idx, 2, acc.z);
}

// ---------------------------------------------------------------------------------------
// Affine epilogue of the BIP-340 and recovery paths.  Both need x/Z^2, y/Z^3 of the ladder's
// result (the reference inverts per point: XBytes / IsYOdd, point_s11n.go:119-134); here one
// thread takes FIN_M pending lanes (strided, so loads coalesce), multiplies their Z together,
// inverts once and walks back (Montgomery's trick): 1 inversion per 16 results.
//   MODE_SCHNORR: valid iff y even and x == r (verifySchnorrSignatureR, schnorr.go:451-478)
//   MODE_RECOVER: writes the 65-byte key record (RecoverPublicKey, ecdsa.go:244-282)
// Lanes that are not pending (already rejected, or queued for the complete kernel) ride along
// with Z = 1.  Scratch: element 3 of the lane's fin region takes the prefix product.
// ---------------------------------------------------------------------------------------

template <int MODE>
__global__ void __launch_bounds__(64)
k_affine_finish(uint32_t n, uint32_t T, const uint8_t* __restrict__ rsig, uint32_t* __restrict__ fin,
                uint8_t* __restrict__ out, size_t stride, uint8_t* __restrict__ out_pts) {
  uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= T) return;
  fe29 acc = fe29_one();
#pragma unroll 1
  for (int j = 0; j < FIN_M; ++j) {
    size_t i = (size_t)t + (size_t)j * T;
    if (i >= n) break;
    if (out[i] == VERDICT_PENDING) acc = fe29_mul(acc, fq_load(fin, stride, i, 2));
    fq_store(fin, stride, i, 3, acc);
  }
  fe29 inv = fe29_inv_gcd(acc);   // safegcd mod p (fe29_inv.h): a quarter of the Fermat chain's instructions, and this kernel is latency bound
#pragma unroll 1
  for (int j = FIN_M - 1; j >= 0; --j) {
    size_t i = (size_t)t + (size_t)j * T;
    if (i >= n || out[i] != VERDICT_PENDING) continue;
    fe29 prev = j > 0 ? fq_load(fin, stride, i - T, 3) : fe29_one();
    fe29 zi = fe29_mul(inv, prev);                     // 1 / Z_i
    inv = fe29_mul(inv, fq_load(fin, stride, i, 2));
    fe29 zi2 = fe29_sqr(zi);
    fe29 x = fe29_mul(fq_load(fin, stride, i, 0), zi2);
    fe29 y = fe29_normalize(fe29_mul(fe29_mul(fq_load(fin, stride, i, 1), zi2), zi));
    if constexpr (MODE == MODE_RECOVER) {
      uint32_t xw[8], yw[8];
      fe29_to_words(xw, fe29_normalize(x));
      fe29_to_words(yw, y);
      uint8_t* rec = out_pts + i * 65;
      rec[0] = 0x04;
      store_be32_unaligned(rec + 1, xw);
      store_be32_unaligned(rec + 33, yw);
      out[i] = 1;
    } else {
      uint32_t rw[8];
      load_be32(rw, rsig + i * 64);
      out[i] = ((y.n[0] & 1u) == 0 && fe29_eq(x, fe29_from_words(rw))) ? 1 : 0;
    }
  }
}

// ---------------------------------------------------------------------------------------
// BIP-340: scalar preparation (no inversion needed: R = s*G + (-e)*P) and complete fallback
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_schnorr_prep(uint32_t n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
               const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
               uint32_t* __restrict__ prep, size_t stride) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  sc s, e;
  bool ok = schnorr_parse(i, pk, sig, msgs, offs, msg_len, s, e);
  sc u2 = sc_neg(e);                                   // schnorr.go:244
  sc k1, k2;
  bool neg1, neg2;
  sc_split_glv_odd(u2, k1, neg1, k2, neg2);
  uint32_t f = (ok ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) |
               (k1.v[4] ? PF_K1_B128 : 0) | (k2.v[4] ? PF_K2_B128 : 0);
#pragma unroll
  for (int w = 0; w < 8; ++w) prep[(size_t)w * stride + i] = s.v[w];
#pragma unroll
  for (int w = 0; w < 4; ++w) prep[(size_t)(8 + w) * stride + i] = k1.v[w];
#pragma unroll
  for (int w = 0; w < 4; ++w) prep[(size_t)(12 + w) * stride + i] = k2.v[w];
  prep[(size_t)16 * stride + i] = f;
}

// ---------------------------------------------------------------------------------------
// u1*G + u2*P for arbitrary (u1, u2, P) through the verification ladder (S2K_IMPL_FAST of
// s2k_double_scalar_mult_basepoint_batch_ex): the same table, signed-digit ladder and generator
// additions as a verification, with the affine result written as a 65-byte record.
//   k_hot_prep          65-byte records -> 64-byte affine points + prep planes (u1, odd GLV
//                       halves of u2); identity / malformed records go straight to the worklist
//   k_verify_fast<MODE_POINT>, k_affine_finish<MODE_RECOVER>
//   k_point_fallback    worklist lanes by the complete path (pt_base_mul + pt_mul_glv)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_hot_prep(uint32_t n, const uint8_t* __restrict__ u1, const uint8_t* __restrict__ u2, const uint8_t* __restrict__ pts65,
           uint8_t* __restrict__ pub64, uint32_t* __restrict__ prep, size_t stride, uint32_t* __restrict__ wl_count,
           uint32_t* __restrict__ wl, uint32_t* __restrict__ status) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* rec = pts65 + i * 65;
  apt a;
  load_be32_unaligned(a.x.v, rec + 1);
  load_be32_unaligned(a.y.v, rec + 33);
  bool finite = rec[0] == 0x04 && fe_is_canonical_raw(a.x.v) && fe_is_canonical_raw(a.y.v) && apt_on_curve(a);
  if (!finite && rec[0] != 0x00) atomicOr(status, 1u);   // not a Point the reference could have built
  if (!finite) {                                          // identity: the complete kernel returns u1*G
    a.x = fe_from_limbs(FE_GX);
    a.y = fe_from_limbs(FE_GY);
    uint32_t pos = atomicAdd(wl_count, 1u);
    wl[pos] = (uint32_t)i;
  }
  store_be32(pub64 + i * 64, a.x.v);
  store_be32(pub64 + i * 64 + 32, a.y.v);
  uint32_t raw[8];
  sc k1, k2;
  bool neg1, neg2;
  load_be32(raw, u1 + i * 32);        // zeros for a plain scalar multiplication
  sc v1 = sc_reduce_once(raw);
  load_be32(raw, u2 + i * 32);
  sc_split_glv_odd(sc_reduce_once(raw), k1, neg1, k2, neg2);
  uint32_t f = (finite ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) | (k1.v[4] ? PF_K1_B128 : 0) |
               (k2.v[4] ? PF_K2_B128 : 0);
#pragma unroll
  for (int w = 0; w < 8; ++w) prep[(size_t)w * stride + i] = v1.v[w];
#pragma unroll
  for (int w = 0; w < 4; ++w) prep[(size_t)(8 + w) * stride + i] = k1.v[w];
#pragma unroll
  for (int w = 0; w < 4; ++w) prep[(size_t)(12 + w) * stride + i] = k2.v[w];
  prep[(size_t)16 * stride + i] = f;
}

// One launcher per kernel: it enqueues on the stream it is given and does nothing else (error checks, events and profiling
// marks stay with the flows).  `ctx` gives the call's generator table (gt_call) and the worklist kernels' grid.
// launch_scalar_prep: signatures [first, first + count) on `lanes` lanes (the planes are linear in the signature index: a piece
// is the same kernel on shifted pointers); launch_ladder: the only place that names an instantiation of k_verify_fast in a
// launch.  The launchers of the fallback and worklist kernels: fallback.hip.
// The launchers of the wave-per-signature and four-lanes-per-signature kernels: small_call.hip.
__attribute__((visibility("hidden"))) void launch_scalar_prep(hipStream_t st, const lane_ws& w, size_t first, size_t count, uint32_t lanes, const uint8_t* dig, const uint8_t* r,
                               const uint8_t* s, const uint8_t* recid, uint32_t flags) {
  k_scalar_prep<<<(lanes + 63) / 64, 64, 0, st>>>((uint32_t)count, lanes, dig + first * 32, r + first * 32, s + first * 32,
                                                  recid ? recid + first : nullptr, flags, w.prep + first, w.pref + first, w.smont + first,
                                                  w.stride);
}
__attribute__((visibility("hidden"))) void launch_generator_part(const s2k_ctx* ctx, hipStream_t st, const lane_ws& w, uint32_t first, uint32_t end) {
  k_generator_part<<<blocks_for(end - first), 256, 0, st>>>(first, end, w.prep, ctx->gt_call, w.gp, w.stride);
}
__attribute__((visibility("hidden"))) void launch_ladder(const s2k_ctx* ctx, hipStream_t st, int mode, size_t n, uint32_t kvf, const uint8_t* pub, const uint8_t* rsig,
                          const lane_ws& w, uint8_t* out, uint8_t* out_pts, uint64_t* clk, const key_groups& kg) {
#define S2K_LADDER(M)                                                                                                              \
  case M:                                                                                                                          \
    k_verify_fast<M><<<blocks_for(n), 256, 0, st>>>((uint32_t)n | kvf, pub, rsig, w.prep, w.qt, w.fin, ctx->gt_call, out, w.wl_count, \
                                                    w.wl, w.stride, out_pts, clk, kg);                                             \
    break;
  // The comb ladders run in a kernel of their own that needs no lead point (comb_ladder.hip: k_verify_comb, same arguments);
  // S2K_COMB_LEAD=1 brings back k_verify_fast<MODE_.._COMB>, =0 the new kernel where the build's default is the old one -
  // read at every call, as S2K_KEY_FINISH_COMB is, so that a process can switch for A/B runs and for the tests that compare
  // the two.  profiles/r20_comb_nolead_ab.txt.
  if (mode == MODE_ECDSA_COMB || mode == MODE_SCHNORR_COMB) {
    const char* lead = getenv("S2K_COMB_LEAD");
    if (!(lead && *lead ? atoi(lead) != 0 : S2K_COMB_LEAD_DEFAULT != 0)) {
      if (mode == MODE_ECDSA_COMB)
        k_verify_comb<false><<<blocks_for(n), 256, 0, st>>>((uint32_t)n | kvf, pub, rsig, w.prep, w.qt, w.fin, ctx->gt_call, out, w.wl_count,
                                                            w.wl, w.stride, out_pts, clk, kg);
      else
        k_verify_comb<true><<<blocks_for(n), 256, 0, st>>>((uint32_t)n | kvf, pub, rsig, w.prep, w.qt, w.fin, ctx->gt_call, out, w.wl_count,
                                                           w.wl, w.stride, out_pts, clk, kg);
      return;
    }
  }
  switch (mode) {
    S2K_LADDER(MODE_ECDSA)
    S2K_LADDER(MODE_SCHNORR)
    S2K_LADDER(MODE_RECOVER)
    S2K_LADDER(MODE_POINT)
    S2K_LADDER(MODE_ECDSA_KEYED)
    S2K_LADDER(MODE_ECDSA_LEFT)
    S2K_LADDER(MODE_SCHNORR_KEYED)
    S2K_LADDER(MODE_SCHNORR_LEFT)
    S2K_LADDER(MODE_ECDSA_KEYSET)
    S2K_LADDER(MODE_ECDSA_KEYSET_JOINT)
    S2K_LADDER(MODE_ECDSA_KEYSET_JOINT5)
    S2K_LADDER(MODE_ECDSA_KEYSET_JOINT6)
    S2K_LADDER(MODE_SCHNORR_KEYSET)
    S2K_LADDER(MODE_SCHNORR_KEYSET_JOINT)
    S2K_LADDER(MODE_SCHNORR_KEYSET_JOINT5)
    S2K_LADDER(MODE_SCHNORR_KEYSET_JOINT6)
    S2K_LADDER(MODE_ECDSA_COMB)
    S2K_LADDER(MODE_SCHNORR_COMB)
    default:   // (a launch of nothing would leave the verdicts as they were and report success)
      fprintf(stderr, "secp256k1_voi_amd: launch_ladder: no ladder of mode %d\n", mode);
      abort();
  }
#undef S2K_LADDER
}
__attribute__((visibility("hidden"))) void launch_affine_finish(hipStream_t st, int mode, size_t n, uint32_t T, const uint8_t* rsig, const lane_ws& w, uint8_t* out,
                                 uint8_t* out_pts) {
  if (mode == MODE_RECOVER)
    k_affine_finish<MODE_RECOVER><<<(T + 63) / 64, 64, 0, st>>>((uint32_t)n, T, rsig, w.fin, out, w.stride, out_pts);
  else
    k_affine_finish<MODE_SCHNORR><<<(T + 63) / 64, 64, 0, st>>>((uint32_t)n, T, rsig, w.fin, out, w.stride, out_pts);
}
__attribute__((visibility("hidden"))) void launch_schnorr_prep(hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs,
                                const uint64_t* offs, uint32_t msg_len) {
  k_schnorr_prep<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, pk, sig, msgs, offs, msg_len, w.prep, w.stride);
}
__attribute__((visibility("hidden"))) void launch_hot_prep(hipStream_t st, size_t n, const lane_ws& w, const uint8_t* u1, const uint8_t* u2, const uint8_t* pts65, uint8_t* pub64,
                            uint32_t* status) {
  k_hot_prep<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, u1, u2, pts65, pub64, w.prep, w.stride, w.wl_count, w.wl, status);
}
