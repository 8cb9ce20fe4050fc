// engine.hip — the lane-per-signature kernels (k_scalar_prep, k_generator_part, k_verify_fast, k_affine_finish, k_schnorr_prep),
// the complete-formula fallback and worklist kernels, the context, and the ECDSA, BIP-340, recovery and point call flows of
// include/secp256k1_voi_amd.h.  Elsewhere: the kernels of calls too small for a lane per signature (small_call.hip); host
// staging, tickets and page-locked memory (pipeline.hip); the generator tables (gtable.hip); key sets and the entry points
// over them (keyset.hip).
//
// One lane per signature / per point; every lane of a wave runs the same instruction
// stream (complete formulas, fixed windows), so there is no divergence on secret- or
// data-dependent branches and no idle lanes.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include <sys/random.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "engine_internal.h"
#include "keyset_index.h"
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

// one signature, complete formulas only (secec/ecdsa.go:392-470)
S2K_DEV uint8_t verify_complete(size_t idx, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ dig,
                                const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig, uint32_t flags,
                                gt_view gt, uint32_t* __restrict__ qt, size_t stride) {
  sc r, s;
  uint32_t e_raw[8];
  apt q;
  load_be32(r.v, rsig + idx * 32);
  load_be32(s.v, ssig + idx * 32);
  load_be32(e_raw, dig + idx * 32);
  load_be32(q.x.v, pub + idx * 64);
  load_be32(q.y.v, pub + idx * 64 + 32);

  // ParseCompactSignature range checks (s11n.go:129-144) + verify step 1 (ecdsa.go:400)
  bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && sc_is_canonical_raw(s.v) && !sc_is_zero(s);
  if (flags & S2K_ECDSA_REJECT_MALLEABLE) ok = ok && !sc_is_gt_half_n(s);   // ecdsa.go:212
  // NewPublicKey: canonical coordinates on the curve (point_s11n.go:187-201)
  ok = ok && fe_is_canonical_raw(q.x.v) && fe_is_canonical_raw(q.y.v) && apt_on_curve(q);

  sc e = sc_reduce_once(e_raw);                    // hashToScalar (ecdsa.go:477-486)
  sc s_inv_m = sc_mont_inv(sc_to_mont(s));         // s^-1 * R
  sc u1 = sc_montmul(e, s_inv_m);                  // e / s   (plain)
  sc u2 = sc_montmul(r, s_inv_m);                  // r / s

  pt rg = pt_base_mul(gt, u1.v);
  pt rq = pt_mul_glv(u2, q, qt, stride, idx);
  pt R = pt_add_complete(rg, rq);                  // point_mul_glv.go:316

  ok = ok && !pt_is_identity(R);                   // ecdsa.go:450
  // x(R) mod n == r  <=>  X == r*Z  or  (r + n < p and X == (r + n)*Z)   (ecdsa.go:459-465)
  fe rf;
#pragma unroll
  for (int i = 0; i < 8; ++i) rf.v[i] = r.v[i];
  bool match = fe_eq(R.x, fe_mul(rf, R.z));
  if (u256_lt(r.v, FE_P_MINUS_N)) {
    fe r2;
    u256_add(r2.v, r.v, SC_N);
    match = match || fe_eq(R.x, fe_mul(r2, R.z));
  }
  return (ok && match) ? 1 : 0;
}

// every lane through the complete path (S2K_ECDSA_FORCE_COMPLETE; also the round-1 baseline kernel)
__global__ void __launch_bounds__(256)
k_ecdsa_verify(uint32_t n, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ dig,
               const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig, uint32_t flags,
               uint8_t* __restrict__ out, gt_view gt, uint32_t* __restrict__ qt, size_t stride) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  out[idx] = verify_complete(idx, pub, dig, rsig, ssig, flags, gt, qt, stride);
}

// ---------------------------------------------------------------------------------------
// The worklist verifier: one signature with COMPLETE formulas on the 9x29 field (pt29.h: the
// Renes-Costello-Batina addition, mixed addition and doubling, point_projective.go:24,123,208).
// Same verdict as verify_complete for every input (tests run both), about a third of its cost:
// lanes whose Jacobian ladder hit an exceptional case are re-done at close to the fast path's own
// speed, so a batch crafted to send EVERY lane here (u1*G + u2*Q = infinity; anyone with a key
// pair can mint those) costs a small multiple of a normal batch instead of serialising on the
// 8x32 reference-shaped path.
// Ladder: odd GLV halves (sc_split_glv_odd), signed odd digits, projective table of the 8 odd
// multiples {1,3,..,15}*Q in planes [entry*27 + limb][lane] of the lane's table region; the
// lambda-half multiplies X by beta at the lookup.
// ---------------------------------------------------------------------------------------
S2K_DEV void p29_store(uint32_t* __restrict__ qt, size_t stride, size_t lane, int entry, const pt29& p) {
  uint32_t* b = qt + (size_t)(entry * 27) * stride + lane;
#pragma unroll
  for (int w = 0; w < 9; ++w) {
    b[(size_t)w * stride] = p.x.n[w];
    b[(size_t)(9 + w) * stride] = p.y.n[w];
    b[(size_t)(18 + w) * stride] = p.z.n[w];
  }
}
S2K_DEV pt29 p29_load(const uint32_t* __restrict__ qt, size_t stride, size_t lane, uint32_t entry) {
  const uint32_t* b = qt + (size_t)(entry * 27) * stride + lane;
  pt29 p;
#pragma unroll
  for (int w = 0; w < 9; ++w) {
    p.x.n[w] = b[(size_t)w * stride];
    p.y.n[w] = b[(size_t)(9 + w) * stride];
    p.z.n[w] = b[(size_t)(18 + w) * stride];
  }
  return p;
}
static_assert(QT_ENTRIES * 27 <= 8 * 8 * 4, "projective 9x29 table must fit in the lane's table region");

// u1*G + u2*Q (Q affine, on the curve) with complete formulas: the projective result (X : Y : Z)
S2K_DEV pt29 dsm_complete29(const sc& u1, const sc& u2, const fe29& qx, const fe29& qy, gt_view gt,
                            uint32_t* __restrict__ qt, size_t stride, size_t idx) {
  sc k1, k2;
  bool neg1, neg2;
  sc_split_glv_odd(u2, k1, neg1, k2, neg2);

  // table of odd multiples (projective): T[j] = (2j + 1) Q
  pt29 q1;
  q1.x = qx;
  q1.y = qy;
  q1.z = fe29_one();
  {
    pt29 q2 = pt29_double(q1), cur = q1;
    p29_store(qt, stride, idx, 0, cur);
#pragma unroll 1
    for (int j = 1; j < QT_ENTRIES; ++j) {
      cur = pt29_add(cur, q2);
      p29_store(qt, stride, idx, j, cur);
    }
  }
  const fe29 beta = fe29_from_words(FE_BETA);
  digit_stream d1 = ds_init(k1), d2 = ds_init(k2);
  // top digits are +1: acc = s1 * Q + s2 * lambda Q
  pt29 acc = q1;
  acc.y = fe29_cond_negate1(qy, neg1);
  acc.y = fe29_normalize_weak(acc.y);
  {
    fe29 bx = fe29_mul(qx, beta);
    acc = pt29_add_mixed(acc, bx, fe29_normalize_weak(fe29_cond_negate1(qy, neg2)));
  }
#pragma unroll 1
  for (int i = 31; i >= 0; --i) {
#pragma unroll 1
    for (int j = 0; j < 4; ++j) acc = pt29_double(acc);
    uint32_t w1 = ds_next(d1), w2 = ds_next(d2);
#pragma unroll 1
    for (int t = 0; t < 2; ++t) {
      uint32_t w = t ? w2 : w1;
      bool neg = (t ? neg2 : neg1) != (w < 8u);
      uint32_t entry = (w < 8u) ? (7u - w) : (w - 8u);
      pt29 a = p29_load(qt, stride, idx, entry);
      if (t) a.x = fe29_mul(a.x, beta);
      a.y = fe29_normalize_weak(fe29_cond_negate1(a.y, neg));
      acc = pt29_add(acc, a);
    }
  }
  // generator part (complete mixed additions; no table entry is the identity)
  {
    uint32_t u[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) u[w] = u1.v[w];
#pragma unroll 1
    for (uint32_t w = 0; w < gt.windows; ++w) {
      apt g = gt_load(gt, w, gt_next_digit(u, gt.bits));
      acc = pt29_add_mixed(acc, fe29_from_words(g.x.v), fe29_from_words(g.y.v));
    }
  }
  return acc;
}

// (the tags of a worklist entry, WL_*: engine_internal.h)

// (`key`: the 64 bytes X || Y of the signature's public key)
S2K_DEV uint8_t verify_complete29(size_t idx, const uint8_t* __restrict__ key, const uint8_t* __restrict__ dig,
                                  const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig, uint32_t flags,
                                  gt_view gt, uint32_t* __restrict__ qt, size_t stride, size_t lane,
                                  uint32_t tag = 0) {
  // idx: the signature; lane: the table column this thread may use (the worklist kernel passes the worklist
  // POSITION, not the signature: the keyed ladder queues signatures in key order, and columns picked by
  // signature would scatter a wave's table accesses over 64 cache lines: 47 ms instead of 20 for a batch
  // that is queued whole)
  sc r, s;
  uint32_t e_raw[8];
  apt q;
  load_be32(r.v, rsig + idx * 32);
  load_be32(s.v, ssig + idx * 32);
  load_be32(e_raw, dig + idx * 32);
  load_be32(q.x.v, key);
  load_be32(q.y.v, key + 32);
  bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && sc_is_canonical_raw(s.v) && !sc_is_zero(s);
  if (flags & S2K_ECDSA_REJECT_MALLEABLE) ok = ok && !sc_is_gt_half_n(s);
  ok = ok && fe_is_canonical_raw(q.x.v) && fe_is_canonical_raw(q.y.v);
  if (!ok) {   // keep the arithmetic well defined; the verdict is already "invalid"
    q.x = fe_from_limbs(FE_GX);
    q.y = fe_from_limbs(FE_GY);
    s = sc_zero();
    s.v[0] = 1;
  }
  fe29 qx = fe29_from_words(q.x.v), qy = fe29_from_words(q.y.v);
  {
    fe29 rhs = fe29_mul(fe29_sqr(qx), qx);
    rhs.n[0] += 7;
    if (!fe29_eq(fe29_sqr(qy), rhs)) {   // not on the curve (point_s11n.go:298-307)
      ok = false;
      qx = fe29_from_words(FE_GX);
      qy = fe29_from_words(FE_GY);
    }
  }
  sc e = sc_reduce_once(e_raw);
  sc26 s_inv_m = sc26_mont_inv(sc26_to_mont(sc26_from_sc(s)));   // s^-1 * R (safegcd, modinv30.h)
  sc u1 = sc26_to_sc(sc26_mm(sc26_from_sc(e), s_inv_m)), u2 = sc26_to_sc(sc26_mm(sc26_from_sc(r), s_inv_m));
  pt29 acc;
  if (tag == WL_DOUBLE_GEN) {
    // the fast ladder has established u2 Q == u1 G (engine.hip, k_verify_fast: verdict): R = 2 u1 G, from the resident
    // tables with the complete formulas - no ladder
    acc.x = fe29_zero();
    acc.y = fe29_one();
    acc.z = fe29_zero();
    uint32_t u[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) u[w] = u1.v[w];
#pragma unroll 1
    for (uint32_t w = 0; w < gt.windows; ++w) {
      apt g = gt_load(gt, w, gt_next_digit(u, gt.bits));
      acc = pt29_add_mixed(acc, fe29_from_words(g.x.v), fe29_from_words(g.y.v));
    }
    acc = pt29_double(acc);
  } else if (tag == WL_DOUBLE_LAST) {
    uint32_t u[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) u[w] = u1.v[w];
    uint32_t digit = 0;
#pragma unroll 1
    for (uint32_t w = 0; w < gt.windows; ++w) digit = gt_next_digit(u, gt.bits);
    apt g = gt_load(gt, gt.windows - 1, digit);
    acc.x = fe29_from_words(g.x.v);
    acc.y = fe29_from_words(g.y.v);
    acc.z = fe29_one();
    acc = pt29_double(acc);
  } else {
    acc = dsm_complete29(u1, u2, qx, qy, gt, qt, stride, lane);
  }
  ok = ok && !fe29_is_zero(acc.z);                   // ecdsa.go:450
  // x(R) mod n == r  <=>  X == r*Z  or  (r + n < p and X == (r + n)*Z)   (ecdsa.go:459-465)
  bool match = fe29_eq(acc.x, fe29_mul(fe29_from_words(r.v), acc.z));
  if (u256_lt(r.v, FE_P_MINUS_N)) {
    uint32_t r2[8];
    u256_add(r2, r.v, SC_N);
    match = match || fe29_eq(acc.x, fe29_mul(fe29_from_words(r2), acc.z));
  }
  return (ok && match) ? 1 : 0;
}

// the lanes the fast kernel could not decide (final Z = 0): a short worklist, normally empty
__global__ void __launch_bounds__(256)
k_verify_fallback(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, const uint8_t* __restrict__ pub,
                  const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig,
                  uint32_t flags, uint8_t* __restrict__ out, gt_view gt, uint32_t* __restrict__ qt,
                  size_t stride) {
  uint32_t count = *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    const uint32_t e = wl[w];
    const size_t idx = e & WL_INDEX_MASK;
    out[idx] = verify_complete29(idx, pub + idx * 64, dig, rsig, ssig, flags, gt, qt, stride, w, e & ~WL_INDEX_MASK);
  }
}
// the same for a batch verified against a key set: the key of signature idx is keys[kidx[idx]]
__global__ void __launch_bounds__(256)
k_verify_fallback_keyset(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, const uint8_t* __restrict__ keys,
                         const uint32_t* __restrict__ kidx, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig,
                         const uint8_t* __restrict__ ssig, uint32_t flags, uint8_t* __restrict__ out, gt_view gt,
                         uint32_t* __restrict__ qt, size_t stride) {
  uint32_t count = *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    const uint32_t e = wl[w];
    const size_t idx = e & WL_INDEX_MASK;
    out[idx] = verify_complete29(idx, keys + (size_t)kidx[idx] * 64, dig, rsig, ssig, flags, gt, qt, stride, w, e & ~WL_INDEX_MASK);
  }
}

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
#ifndef S2K_PREP_M
#define S2K_PREP_M 6
#endif
constexpr int PREP_M = S2K_PREP_M;
constexpr int PREP_WORDS = 17;
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
// Fast path, kernel 2: per-lane table, ladder, generator part, final comparison.
// Per-lane table {1,3,..,15}*Q brought to one common Z (no inversion): build A_j = A_{j-1} + 2Q
// on the curve isomorphic by C = Z(2Q), remember H_j (Z_j = Z_{j-1} H_j), then scale entry j
// by (H_{j+1}...H_7)^{2,3}.  The ladder then only ever adds affine points (8 M + 3 S); its
// result has the true Z = Z_ladder * Z_7 * C.
// Table storage: tb_* (lane_tables.h).  Z_7 * C and the results handed to k_affine_finish go to the lane's
// "fin" elements.
// ---------------------------------------------------------------------------------------

// Waves per SIMD the joint-table key-set ladder is built for.  Measured (tools/gpu_joint_waves.sh, same box, two runs each):
// 3 waves (150 VGPRs, no spills) 1.743 / 1.746 ms, 4 waves (128 VGPRs, 21 spilled) 1.733 / 1.743 ms - the kernel is at the
// clock the chip gives it (1.89-2.02 GHz under 8 GB of table fetches per launch) either way; 3 stays.
#ifndef S2K_JOINT_WAVES
#define S2K_JOINT_WAVES 3
#endif
// (the comb ladders' bound, S2K_COMB_WAVES, and VERDICT_PENDING: engine_internal.h)

// Digits of an odd half scalar k < 2^129 in the order the per-key ladder consumes them.  As in
// ds_init, digit i is nib_i = bits 4i+1 .. 4i+4 of k (signed value 2 nib_i - 15); digit i = 4c + j
// belongs to chunk c = 2^(16c) Q and round j, and the ladder runs round 3 first, chunks upwards: its
// nibble goes to place (3 - j) * 8 + c from the top of a 128-bit stream.
struct digit_stream4 {
  uint32_t w[4];
};
S2K_DEV digit_stream4 ds4_init_chunked(const sc& k_odd) {
  digit_stream4 d;
  d.w[0] = d.w[1] = d.w[2] = d.w[3] = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int bit = 4 * i + 1, limb = bit >> 5, sh = bit & 31;
    uint32_t nib = k_odd.v[limb] >> sh;
    if (sh > 28) nib |= k_odd.v[limb + 1] << (32 - sh);
    nib &= 15u;
    const int c = i >> 2, j = i & 3, pos = 124 - 4 * ((3 - j) * 8 + c);
    d.w[pos >> 5] |= nib << (pos & 31);
  }
  return d;
}
S2K_DEV uint32_t ds4_next(digit_stream4& d) {
  uint32_t nib = d.w[3] >> 28;
  d.w[3] = (d.w[3] << 4) | (d.w[2] >> 28);
  d.w[2] = (d.w[2] << 4) | (d.w[1] >> 28);
  d.w[1] = (d.w[1] << 4) | (d.w[0] >> 28);
  d.w[0] <<= 4;
  return nib;
}

// MODE_ECDSA:   pub = n x 64 (X||Y), rsig = n x 32 (r);      accept iff x(R) mod n == r
// MODE_SCHNORR: pub = n x 32 (x-only key, BIP-340), rsig = n x 64 signatures (r at offset 0);
//               P = lift_x(pub) (NewSchnorrPublicKey, schnorr.go:257-275), accept iff R != inf,
//               y(R) even and x(R) == r (verifySchnorrSignatureR, schnorr.go:451-478)
// MODE_RECOVER: pub unused, rsig = n x 32 (r); the point is R = RecoverPoint(r, id) with the id
//               from the prep flag word; out = ok bytes, out_pts = n x 65 records of
//               Q = (-e/r) G + (s/r) R (RecoverPublicKey, ecdsa.go:244-282)
// MODE_POINT:   pub = n x 64 (X||Y), rsig unused; out_pts = n x 65 records of u1*G + u2*P with
//               u1 and the split u2 taken from the prep planes as they are
//               (DoubleScalarMultBasepointVartime, point_mul_glv.go:307; k_hot_prep)
// MODE_ECDSA_KEYED / MODE_ECDSA_LEFT: MODE_ECDSA after the batch has been grouped by public key
//               (keyed.hip).  Lane idx < *kg.counters[...] handles signature perm[idx]: inputs, prep
//               planes and the verdict are the signature's, workspace columns are the lane's.
//               KEYED lanes take their points from the key's precomputed affine table (table ptab[idx],
//               no per-lane table, 12 doublings); LEFT lanes are the general path for the rest.
// MODE_ECDSA_COMB: MODE_ECDSA_KEYED over the comb tables an ECDSA call builds by default (keyed.hip: k_key_chain on the comb's
//               geometry, k_key_finish_comb): the same 64 entries per key serve 7 bits of a half scalar per addition.
// MODE_SCHNORR_KEYED / MODE_SCHNORR_LEFT: the same for BIP-340 (tables of the lifted x-only keys); results go
//               to k_affine_finish in the SIGNATURE's fin column.
// MODE_SCHNORR_COMB: MODE_SCHNORR_KEYED over comb tables.  kg.key_bytes == 32: the tables of a call's lifted x-only keys;
//               kg.key_bytes == 64: a comb key set (S2K_KEYSET_COMB), pub = the set's X || Y keys - an odd Y flips both half
//               scalars' signs, as in the MODE_SCHNORR_KEYSET modes.
// Waves per SIMD the register allocator must leave room for.  Measured (2^20 signatures):
// unbounded (240 VGPRs, 2 waves) 11.08 ms; 3 waves (168 VGPRs, no spills) 10.89 ms; 4 waves
// (128 VGPRs, 96 spilled) 11.45 ms.
#ifndef S2K_FAST_WAVES
#define S2K_FAST_WAVES 3
#endif
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

template <int MODE>
#ifdef S2K_FAST_MAX_WAVES   // experiment: cap the occupancy (leaves VGPRs for a kernel of another stream to run beside the ladder)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(S2K_FAST_MAX_WAVES, S2K_FAST_MAX_WAVES)))
#else
// (The ladders over per-key tables hold no per-lane table state and come out at 126 VGPRs: four waves per SIMD.  That is
// the allocator's doing under a bound of three, and it is fragile: a rare branch that kept the accumulator alive across the
// final addition took 152, and asking for four waves outright spills - 26 VGPRs for <ECDSA_KEYED>, 28 for the key-set
// ladder, which stays at 142 VGPRs and three waves.  tests/test_counts_cpu.py watches the instruction counts; the
// resource usage is printed by tools/kernel_regs.sh.)
__global__ void __launch_bounds__(256, (MODE == MODE_ECDSA_KEYSET_JOINT || MODE == MODE_ECDSA_KEYSET_JOINT5 || MODE == MODE_ECDSA_KEYSET_JOINT6 ||
                                        MODE == MODE_SCHNORR_KEYSET_JOINT || MODE == MODE_SCHNORR_KEYSET_JOINT5 || MODE == MODE_SCHNORR_KEYSET_JOINT6)
                                           ? S2K_JOINT_WAVES : (MODE == MODE_ECDSA_COMB || MODE == MODE_SCHNORR_COMB) ? S2K_COMB_WAVES : S2K_FAST_WAVES)
#endif
k_verify_fast(uint32_t n_and_flags, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ rsig,
              const uint32_t* __restrict__ prep, uint32_t* __restrict__ qt, uint32_t* __restrict__ fin,
              gt_view gt, uint8_t* __restrict__ out, uint32_t* __restrict__ wl_count,
              uint32_t* __restrict__ wl, size_t stride, uint8_t* __restrict__ out_pts, uint64_t* __restrict__ clk,
              key_groups kg) {
  constexpr bool SKS = MODE >= MODE_SCHNORR_KEYSET && MODE <= MODE_SCHNORR_KEYSET_JOINT6;   // BIP-340 over a key set
  constexpr int KM = SKS ? MODE - 4 : MODE;                  // the key-set layout, as its ECDSA mode
  constexpr bool JOINT = KM == MODE_ECDSA_KEYSET_JOINT;      // ... over its joint tables: one addition per digit position
  constexpr int JW = KM == MODE_ECDSA_KEYSET_JOINT5 ? 5 : KM == MODE_ECDSA_KEYSET_JOINT6 ? 6 : 4;
  constexpr bool JOINTW = JW > 4;                            // ... over joint tables of 5- or 6-bit digits (kjw_geom: 26 / 22 positions)
  constexpr bool KEYSET = KM == MODE_ECDSA_KEYSET || JOINT || JOINTW;   // KEYED over a key set's 32-chunk tables: no doublings at all
  constexpr bool COMB = MODE == MODE_ECDSA_COMB || MODE == MODE_SCHNORR_COMB;   // KEYED over the comb table of the key
  constexpr bool KEYED = MODE == MODE_ECDSA_KEYED || MODE == MODE_SCHNORR_KEYED || KEYSET || COMB;
  constexpr bool GROUPED = KEYED || MODE == MODE_ECDSA_LEFT || MODE == MODE_SCHNORR_LEFT;
  constexpr bool ECDSA = MODE == MODE_ECDSA || MODE == MODE_ECDSA_KEYED || MODE == MODE_ECDSA_LEFT || (KEYSET && !SKS) || MODE == MODE_ECDSA_COMB;
  const bool force_wl = (n_and_flags & KVF_FORCE_WORKLIST) != 0;
  const uint32_t n = n_and_flags & ~KVF_FORCE_WORKLIST;
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;         // lane: workspace column
  size_t sig = idx;                                            // signature: input / prep / verdict column
  uint32_t lanes = n;
  if constexpr (GROUPED) {
    uint32_t lo = 0, hi = kg.counters[KEYED ? KG_NKEYED : KG_NLEFT];
    if (KEYED && kg.nparts > 1) {                              // two-part flow: this launch takes one side of the split
      const uint32_t sp = kg.counters[KG_SPLIT_LANE];
      if (kg.part) lo = sp;
      else hi = sp;
    }
    idx += lo;
    if (idx >= hi) return;
    lanes = hi - lo;
    sig = (KEYED ? kg.perm : kg.left)[idx];
  } else {
    if (idx >= n) return;
  }
  // effective shader clock of this launch (bench.py roofline): wave 0 of workgroup 0 stamps the
  // shader cycle counter and the constant-rate wall clock when it starts and when it ends
  // (and wave 0 of the LAST workgroup, which runs in the launch's final round: the clock sags under power
  // over the 8 ms of a launch)
  const bool stamp = clk != nullptr && (blockIdx.x == 0 || blockIdx.x == (lanes - 1) / 256) && threadIdx.x < 64;
  uint64_t t0c = 0, t0w = 0;
  if (stamp) {
    t0c = __builtin_readcyclecounter();
    t0w = __builtin_amdgcn_s_memrealtime();
  }
  uint32_t pf = prep[(size_t)16 * stride + sig];
  bool ok;
  fe29 qx, qy;
  if constexpr (KEYED) {
    ok = (pf & PF_OK) && kg.tinfo[kg.ptab[idx]];      // the key was validated when its table was built
  } else if constexpr (MODE == MODE_RECOVER) {
    uint32_t xw[8];
    load_be32(xw, rsig + idx * 32);
    ok = (pf & PF_OK) != 0;
    if (ok && (pf & 0x200u)) u256_add(xw, xw, SC_N);   // x = r + n (< p, checked by the prep kernel)
    if (!ok) {
#pragma unroll
      for (int i = 0; i < 8; ++i) xw[i] = FE_GX[i];
    }
    qx = fe29_from_words(xw);
    fe29 rhs = fe29_mul(fe29_sqr(qx), qx);
    rhs.n[0] += 7;
    bool has = fe29_sqrt(qy, rhs);                      // SetCompressedBytes (point_s11n.go:152-169)
    if (!has) {
      ok = false;
      qx = fe29_from_words(FE_GX);
      qy = fe29_from_words(FE_GY);
    }
    qy = fe29_normalize(qy);
    bool want_odd = (pf & 0x100u) != 0;
    qy = fe29_select(((qy.n[0] & 1u) != 0) != want_odd, qy, fe29_normalize_weak(fe29_negate(qy, 1)));
  } else if constexpr (ECDSA || MODE == MODE_POINT) {
    apt q;
    load_be32(q.x.v, pub + sig * 64);
    load_be32(q.y.v, pub + sig * 64 + 32);
    ok = (pf & PF_OK) && fe_is_canonical_raw(q.x.v) && fe_is_canonical_raw(q.y.v);
    if (!ok) {   // keep the arithmetic on the curve; the verdict is already "invalid"
      q.x = fe_from_limbs(FE_GX);
      q.y = fe_from_limbs(FE_GY);
    }
    qx = fe29_from_words(q.x.v);
    qy = fe29_from_words(q.y.v);
    // y^2 == x^3 + 7 (point_s11n.go:298-307)
    fe29 rhs = fe29_mul(fe29_sqr(qx), qx);
    rhs.n[0] += 7;
    bool on = fe29_eq(fe29_sqr(qy), rhs);
    if (!on) {
      ok = false;
      qx = fe29_from_words(FE_GX);
      qy = fe29_from_words(FE_GY);
    }
  } else {
    uint32_t xw[8];
    load_be32(xw, pub + sig * 32);
    ok = (pf & PF_OK) && fe_is_canonical_raw(xw);
    if (!ok) {
#pragma unroll
      for (int i = 0; i < 8; ++i) xw[i] = FE_GX[i];
    }
    qx = fe29_from_words(xw);
    fe29 rhs = fe29_mul(fe29_sqr(qx), qx);
    rhs.n[0] += 7;                                    // [1] (+7 on limb 0)
    bool has = fe29_sqrt(qy, rhs);
    if (!has) {   // not an x-coordinate of the curve
      ok = false;
      qx = fe29_from_words(FE_GX);
      qy = fe29_from_words(FE_GY);
    }
    qy = fe29_normalize(qy);
    qy = fe29_select((qy.n[0] & 1u) != 0, qy, fe29_normalize_weak(fe29_negate(qy, 1)));   // even y
  }
  bool neg1 = pf & PF_NEG1, neg2 = pf & PF_NEG2;
  if constexpr (SKS) {
    // BIP-340 multiplies P = lift_x(x), the point with EVEN y; the set holds the key as its caller gave it (X || Y): an odd Y
    // means P = -Q, i.e. both half scalars change sign (`pub`: the set's key array)
    const bool y_odd = (pub[(size_t)kg.ptab[idx] * 64 + 63] & 1u) != 0;
    neg1 = neg1 != y_odd;
    neg2 = neg2 != y_odd;
  }
  if constexpr (MODE == MODE_SCHNORR_COMB) {
    // a comb key set holds X || Y as well (the same flip); the tables of a call are those of the lifted keys: nothing to do.
    // One mode for both: the test is uniform over the launch
    if (kg.key_bytes == 64) {
      const bool y_odd = (pub[(size_t)kg.ptab[idx] * 64 + 63] & 1u) != 0;
      neg1 = neg1 != y_odd;
      neg2 = neg2 != y_odd;
    }
  }

  // ---- table ----
  if constexpr (!KEYED) {
    jpt29 a0;
    a0.x = qx;
    a0.y = qy;
    a0.z = fe29_one();
    jpt29 d = jpt29_double(a0);                      // x [1] y [2] z [1]
    fe29 c2 = fe29_sqr(d.z);
    fe29 c3 = fe29_mul(c2, d.z);
    const fe29 dx = d.x, dy = d.y;                   // the affine addend on the isomorphic curve
    jpt29 cur;
    cur.x = fe29_mul(qx, c2);
    cur.y = fe29_mul(qy, c3);
    cur.z = fe29_one();
    tb_store(qt, stride, idx, 0, TB_X, cur.x);
    tb_store(qt, stride, idx, 0, TB_Y, cur.y);
#pragma unroll 1
    for (int j = 1; j < QT_ENTRIES; ++j) {
      fe29 h;
      cur = jpt29_add_affine(cur, dx, dy, &h);
      tb_store(qt, stride, idx, j, TB_X, cur.x);
      tb_store(qt, stride, idx, j, TB_Y, cur.y);
      tb_store(qt, stride, idx, j, TB_BX, h);          // H_j, replaced by beta * x_j below
    }
    fq_store(fin, stride, idx, TB_ZC_ELEM, fe29_mul(cur.z, d.z));   // Z_7 * C
    fe29 prev_x = cur.x;
    const fe29 beta = fe29_from_words(FE_BETA);
    fe29 rr = fe29_one();
#pragma unroll 1
    for (int j = QT_ENTRIES - 2; j >= 0; --j) {
      rr = fe29_mul(rr, tb_load(qt, stride, idx, j + 1, TB_BX));
      tb_store(qt, stride, idx, j + 1, TB_BX, fe29_mul(prev_x, beta));
      fe29 r2 = fe29_sqr(rr);
      fe29 r3 = fe29_mul(r2, rr);
      prev_x = fe29_mul(tb_load(qt, stride, idx, j, TB_X), r2);
      fe29 y = fe29_mul(tb_load(qt, stride, idx, j, TB_Y), r3);
      tb_store(qt, stride, idx, j, TB_X, prev_x);
      tb_store(qt, stride, idx, j, TB_Y, y);
    }
    tb_store(qt, stride, idx, 0, TB_BX, fe29_mul(prev_x, beta));
  }

  // ---- ladder over |k1|, |k2| ----
  sc k1 = sc_zero(), k2 = sc_zero();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    k1.v[w] = prep[(size_t)(8 + w) * stride + sig];
    k2.v[w] = prep[(size_t)(12 + w) * stride + sig];
  }
  k1.v[4] = (pf & PF_K1_B128) ? 1u : 0u;   // odd by construction (sc_split_glv_odd): the signed
  k2.v[4] = (pf & PF_K2_B128) ? 1u : 0u;   // odd-digit recoding is exact, no final correction
  jpt29 acc;
  if constexpr (COMB) {
    // The comb ladder (kc_geom, engine_internal.h).  k = 2^133 + sum_{i<133} b_i 2^i, b_i = 2 a_i - 1, a = k >> 1 (k odd,
    // < 2^129: a has 128 bits).  Column j (18 down to 0) of a half is the bits a_(19 t + j) of the seven teeth t: the top
    // tooth gives the sign, the lower six (complemented under a negative top tooth) the entry
    // E[idx] = B_6 + sum_{t<6} (2 idx_t - 1) B_t.  A round is one doubling (none in front of the first round) and the two
    // halves' additions: 38 additions and 18 doublings.  The lead 2^133 Q = 2^18 * 2^115 Q goes in first, for both halves at
    // once (L +- phi(L), as in the window ladder).
    // All in Jacobian coordinates, a round's two entries added to each other first: 19 * 20 + 18 * 7 = 506 products (two
    // mixed additions a round: 19 * 22 + 18 * 7 = 544).  XYZZ additions (10 in 9 reductions) would want an XYZZ
    // doubling (6 M + 3 S = 9: 542 products) or the change of form around every single doubling (4 products a round: 578),
    // and a fourth coordinate in registers; jacobian29.h's pair is the one the general ladder runs and the models bound.
    // Z = 0 is sticky through all of it (Z3 = Z1 H h, Z3 = Y Z) and ends on the worklist exactly as before.
    using G = kc_geom;
    const uint4* kt = kg.ktab + (size_t)kg.ptab[idx] * (G::SLOTS * 8);
    {
      fe29 lx, ly;
      ke_load_xy(kt + (size_t)(neg1 == neg2 ? G::LEAD : G::LEAD + 1) * 8, false, lx, ly);
      acc.x = lx;
      acc.y = fe29_cond_negate1(ly, neg1);
      acc.z = fe29_one();
    }
    // tooth t of a half: bits 19 t .. 19 t + 18 of a = k >> 1 (tooth 6: 14 bits and zeros); bit j of it is a shift and a mask.
    // The 19 columns of both halves (7 + 7 bits) are cut once and wait in LDS, one word per round and lane ([round][lane]: no
    // two lanes of a wave share a bank, no lane reads another's): 19 KiB per block, and no register held across the ladder.
    __shared__ uint32_t cols[G::SPACING][256];
    {
      uint32_t t1[G::TEETH], t2[G::TEETH];
#pragma unroll
      for (int t = 0; t < G::TEETH; ++t) {
        const int bit = G::SPACING * t + 1, limb = bit >> 5, sh = bit & 31;      // (+ 1: a = k >> 1)
        uint32_t v1 = k1.v[limb] >> sh, v2 = k2.v[limb] >> sh;
        if (sh > 32 - G::SPACING) {
          v1 |= k1.v[limb + 1] << (32 - sh);
          v2 |= k2.v[limb + 1] << (32 - sh);
        }
        t1[t] = v1 & ((1u << G::SPACING) - 1u);
        t2[t] = v2 & ((1u << G::SPACING) - 1u);
      }
#pragma unroll
      for (int j = 0; j < G::SPACING; ++j) {
        uint32_t w = 0;
#pragma unroll
        for (int t = 0; t < G::TEETH; ++t) w |= (((t1[t] >> j) & 1u) << t) | (((t2[t] >> j) & 1u) << (8 + t));
        cols[j][threadIdx.x] = w;
      }
    }
#pragma unroll 1
    for (int j = G::SPACING - 1;; --j) {
      // the column: E1 of the first half and phi(E2) of the second (the beta * x column) are affine over the same Z, so
      // they are added to each other first (jacobian29.h: coz29_pair_sum, E2 with its sign relative to E1's) and their
      // sum, over Z h, goes to the accumulator moved onto that curve: 15 M + 5 S against the 16 M + 6 S of two mixed
      // additions, and both lookups of the column in flight together
      const uint32_t w12 = cols[j][threadIdx.x], w1 = w12 & 127u, w2 = w12 >> 8;
      const bool top1 = (w1 & 64u) != 0, top2 = (w2 & 64u) != 0;
      const bool n1 = neg1 != !top1, n2 = neg2 != !top2;
      fe29 x1, y1, x2, y2;
      ke_load_xy(kt + (size_t)((top1 ? w1 : ~w1) & 63u) * 8, false, x1, y1);
      ke_load_xy(kt + (size_t)((top2 ? w2 : ~w2) & 63u) * 8, true, x2, y2);
      const coz29_sum t = coz29_pair_sum(x1, y1, x2, fe29_cond_negate1(y2, n1 != n2));
      acc = jpt29_rescale(acc, t.hh, t.hhh);
      acc = jpt29_add_affine(acc, t.x, fe29_cond_negate1(t.ny, !n1));   // (ny = -Y_T)
      acc.z = fe29_mul(acc.z, t.h);
      if (j == 0) break;
      acc = jpt29_double(acc);
    }
    // the table's points are affine on the curve isomorphic by W (keyed.hip): back on secp256k1 itself
    // (W is asked for here and not in front of the ladder: nothing is held across it but the accumulator - neither W's nine
    // registers nor the teeth, which wait in LDS.  The column's four coordinates and its pair sum are 145 VGPRs, three waves
    // per SIMD; bounded to four, S2K_COMB_WAVES=4, the kernel spills 23 and loses what the column saves.)
    acc.z = fe29_mul(acc.z, ke_load(kt + (size_t)G::WENT * 8, G::W));
  } else if constexpr (KEYED) {
    // k = 16^32 + sum_i d_i 16^i with d_i = 2 nib_i - 15, i = 4c + j: round j (3 down to 0) adds
    // d_(4c+j) * 2^(16c) Q for the eight chunks c, with four doublings between rounds; the leading
    // 16^32 Q = 16^3 * 2^116 Q goes in first (for both halves at once: one table point, see below).
    using G = kt_geom<KEYSET ? KS_CHUNKS : KT_CHUNKS>;
    const uint4* kt = kg.ktab + (size_t)kg.ptab[idx] * (G::SLOTS * 8);
    const fe29 kw = ke_load(kt + (size_t)(G::SCR + G::W_SLOT / 3) * 8, G::W_SLOT % 3);   // wanted at the very end: asked for early
    // The 64 additions of this ladder run in XYZZ coordinates (xyzz29.h: 8 M + 2 S in 9 reductions against 8 M + 3 S in
    // 10 for the Jacobian mixed addition: 1 441 instead of 1 578 instructions); the 12 doublings stay Jacobian (7 products
    // against 9), so the accumulator changes form at the three round borders (3 M + 1 S each way together).  The
    // exceptional-case rule carries over: equal x makes ZZ = 0, ZZ = 0 is sticky through additions, conversions and
    // doublings, and ends as Z = 0 -> worklist.
    xyzz29 xa;
    {
      // +-L +- phi(L): the table holds L + phi(L) and L - phi(L) (keyed.hip), the other two are their negatives
      // (wide joint tables: L = 2^(W POS) Q, the pair behind the positions of the key's joint table)
      fe29 lx, ly;
      if constexpr (JOINTW)
        jw_load(kg.jtab + (size_t)kg.ptab[idx] * kjw_geom<JW>::KEY_QUADS + (kjw_geom<JW>::LEAD + (neg1 == neg2 ? 0 : 1)) * kjw_geom<JW>::EQ, lx, ly);
      else
        ke_load_xy(kt + (size_t)(neg1 == neg2 ? G::LEAD : G::LEAD + 1) * 8, false, lx, ly);
      xa = xyzz29_from_affine(lx, fe29_cond_negate1(ly, neg1));
    }
    if constexpr (KEYSET) {
      // Key sets: one chunk per digit, {1,3,..,15} * 16^i Q for i < 32 and L = 16^32 Q: k = 16^32 + sum d_i 16^i is 64
      // table additions, in any order - bottom up, nibble i = bits 4i+1 .. 4i+4 of the odd half scalar (k >> 1, 128 bits).
      // JOINT tables hold, per position, E_a + s phi(E_b) for all pairs of odd multiples and both signs: the two halves'
      // digits d1 = +-(2a+1), d2 = +-(2b+1) are ONE addition of +-(E_a + s phi(E_b)), s = the product of their signs.
      uint32_t a[4], b[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        a[w] = (k1.v[w] >> 1) | (k1.v[w + 1] << 31);
        b[w] = (k2.v[w] >> 1) | (k2.v[w + 1] << 31);
      }
      [[maybe_unused]] const uint4* jt = JOINT ? kg.jtab + (size_t)kg.ptab[idx] * KJ_KEY_QUADS
                                        : JOINTW ? kg.jtab + (size_t)kg.ptab[idx] * kjw_geom<JW>::KEY_QUADS : nullptr;
      if constexpr (JOINTW) {
        // W-bit digits: w_i = bits W i .. W i + W - 1 of (k - 1) / 2, d_i = 2 w_i - (2^W - 1): below 2^(W-1) negative with
        // magnitude 2 (NE - 1 - w) + 1, else positive with magnitude 2 (w - NE) + 1
        using J = kjw_geom<JW>;
        constexpr uint32_t WM = (1u << JW) - 1u, NE = (uint32_t)J::NE;
        // The entry of position c + 1 is asked for BEFORE the addition of position c (measured both ways, profiles/r06_keyset_wait.json): a joint
        // table is 0.8 / 2.75 MiB per key and a lookup is a 64-byte read from HBM more often than not - issued behind the
        // addition, its latency stood between every two additions of a wave.
        auto next_entry = [&](int c, bool& n1_out) -> uint32_t {
          const uint32_t w1 = a[0] & WM, w2 = b[0] & WM;
#pragma unroll
          for (int w = 0; w < 3; ++w) {
            a[w] = (a[w] >> JW) | (a[w + 1] << (32 - JW));
            b[w] = (b[w] >> JW) | (b[w + 1] << (32 - JW));
          }
          a[3] >>= JW;
          b[3] >>= JW;
          const bool n1 = neg1 != (w1 < NE), n2 = neg2 != (w2 < NE);
          const uint32_t ea = (w1 < NE) ? (NE - 1u - w1) : (w1 - NE), eb = (w2 < NE) ? (NE - 1u - w2) : (w2 - NE);
          n1_out = n1;
          return (((uint32_t)c * NE + ea) * NE + eb) * 2u + (n1 != n2 ? 1u : 0u);
        };
        bool n1_cur;
        jw_raw raw = jw_fetch(jt + (size_t)next_entry(0, n1_cur) * J::EQ);
#pragma unroll 1
        for (int c = 0; c < J::POS; ++c) {
          const jw_raw cur = raw;
          const bool n1 = n1_cur;
          if (c + 1 < J::POS) raw = jw_fetch(jt + (size_t)next_entry(c + 1, n1_cur) * J::EQ);
          fe29 x, y;
          jw_point(cur, x, y);
          xa = xyzz29_add_affine(xa, x, fe29_cond_negate1(y, n1));
        }
      } else if constexpr (JOINT) {
        // the 4-bit joint ladder with the same lead: the 80-byte entry of position c + 1 (18 limbs) asked for before the addition
        // of position c
        auto next_entry4 = [&](int c, bool& n1_out) -> uint32_t {
          const uint32_t w1 = a[0] & 15u, w2 = b[0] & 15u;
#pragma unroll
          for (int w = 0; w < 3; ++w) {
            a[w] = (a[w] >> 4) | (a[w + 1] << 28);
            b[w] = (b[w] >> 4) | (b[w + 1] << 28);
          }
          a[3] >>= 4;
          b[3] >>= 4;
          const bool n1 = neg1 != (w1 < 8u), n2 = neg2 != (w2 < 8u);
          const uint32_t ea = (w1 < 8u) ? (7u - w1) : (w1 - 8u), eb = (w2 < 8u) ? (7u - w2) : (w2 - 8u);
          n1_out = n1;
          return (((uint32_t)c * 8u + ea) * 8u + eb) * 2u + (n1 != n2 ? 1u : 0u);
        };
        bool n1_nxt;
        fe29 nx, ny;
        je_load(jt + (size_t)next_entry4(0, n1_nxt) * KJ_ENTRY_QUADS, nx, ny);
#pragma unroll 1
        for (int c = 0; c < KS_CHUNKS; ++c) {
          const fe29 x = nx, y = ny;
          const bool n1 = n1_nxt;
          if (c + 1 < KS_CHUNKS) je_load(jt + (size_t)next_entry4(c + 1, n1_nxt) * KJ_ENTRY_QUADS, nx, ny);
          xa = xyzz29_add_affine(xa, x, fe29_cond_negate1(y, n1));
        }
      } else {
#pragma unroll 1
        for (int c = 0; c < KS_CHUNKS; ++c) {
          const uint32_t w1 = a[0] & 15u, w2 = b[0] & 15u;
#pragma unroll
          for (int w = 0; w < 3; ++w) {
            a[w] = (a[w] >> 4) | (a[w + 1] << 28);
            b[w] = (b[w] >> 4) | (b[w + 1] << 28);
          }
          a[3] >>= 4;
          b[3] >>= 4;
#pragma unroll 1
          for (int t = 0; t < 2; ++t) {
            uint32_t w = t ? w2 : w1;
            bool neg = (t ? neg2 : neg1) != (w < 8u);
            uint32_t entry = (w < 8u) ? (7u - w) : (w - 8u);
            fe29 x, y;
            ke_load_xy(kt + (size_t)(c * 8 + entry) * 8, t != 0, x, y);
            xa = xyzz29_add_affine(xa, x, fe29_cond_negate1(y, neg));
          }
        }
      }
    } else {
      digit_stream4 d1 = ds4_init_chunked(k1), d2 = ds4_init_chunked(k2);
#pragma unroll 1
      for (int round = 0; round < 4; ++round) {
        if (round) {
          jpt29 j4 = xyzz29_to_jacobian(xa);
#pragma unroll 1
          for (int j = 0; j < 4; ++j) j4 = jpt29_double(j4);
          xa = xyzz29_from_jacobian(j4);
        }
#pragma unroll 1
        for (int c = 0; c < KT_CHUNKS; ++c) {
          uint32_t w1 = ds4_next(d1), w2 = ds4_next(d2);
#pragma unroll 1
          for (int t = 0; t < 2; ++t) {
            uint32_t w = t ? w2 : w1;
            bool neg = (t ? neg2 : neg1) != (w < 8u);
            uint32_t entry = (w < 8u) ? (7u - w) : (w - 8u);
            fe29 x, y;
            ke_load_xy(kt + (size_t)(c * 8 + entry) * 8, t != 0, x, y);
            xa = xyzz29_add_affine(xa, x, fe29_cond_negate1(y, neg));
          }
        }
      }
      // (the next entry asked for before the current addition - what the key-set ladders do - costs this ladder its fourth wave
      // per SIMD: 145-147 VGPRs against 126.  Measured in both forms, four alternating pairs: the step 4.89 against 4.91 ms,
      // the kernel 58.2 M against 57.8 M cycles under the counters - nothing, and not kept; profiles/r06_wait_shares.txt)
    }
    acc = xyzz29_to_jacobian(xa);
    // the table's points are affine on the curve isomorphic by W (keyed.hip): back on secp256k1 itself
    acc.z = fe29_mul(acc.z, kw);
  } else {
    digit_stream d1 = ds_init(k1), d2 = ds_init(k2);
    {
      fe29 t0x = tb_load(qt, stride, idx, 0, TB_X), t0y = tb_load(qt, stride, idx, 0, TB_Y), t0bx = tb_load(qt, stride, idx, 0, TB_BX);
      acc.x = t0x;
      acc.y = fe29_cond_negate1(t0y, neg1);
      acc.z = fe29_one();
      acc = jpt29_add_affine(acc, t0bx, fe29_cond_negate1(t0y, neg2));
    }
#pragma unroll 1
    for (int i = 31; i >= 0; --i) {
#pragma unroll 1
      for (int j = 0; j < 4; ++j) acc = jpt29_double(acc);
      uint32_t w1 = ds_next(d1), w2 = ds_next(d2);
#pragma unroll 1
      for (int t = 0; t < 2; ++t) {
        uint32_t w = t ? w2 : w1;
        bool neg = (t ? neg2 : neg1) != (w < 8u);
        uint32_t entry = (w < 8u) ? (7u - w) : (w - 8u);
        fe29 x, y;
        tb_load_xy(qt, stride, idx, entry, t != 0, x, y);
        acc = jpt29_add_affine(acc, x, fe29_cond_negate1(y, neg));
      }
    }
    acc.z = fe29_mul(acc.z, fq_load(fin, stride, idx, TB_ZC_ELEM));   // times Z_7 * C: back on secp256k1 itself
  }

  // ---- generator part: u1*G from the resident tables ----
  // (final_only: Z was not 0 BEFORE the last addition and the addend is finite - then a zero after it arose in that addition,
  // and the verdict code below decides it instead of queueing the lane for the complete-formula kernel)
  bool final_only = false;
  if constexpr (GROUPED) {
    jpt29 q;                                            // computed by k_generator_part
    q.x = fq_load(kg.gp, stride, sig, 0);
    q.y = fq_load(kg.gp, stride, sig, 1);
    q.z = fq_load(kg.gp, stride, sig, 2);
    if constexpr (ECDSA) final_only = !fe29_is_zero(acc.z) && !fe29_is_zero(q.z);
    acc = jpt29_add(acc, q);
  } else {
    uint32_t u[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) u[w] = prep[(size_t)w * stride + sig];
#pragma unroll 1
    for (uint32_t w = 0; w + 1 < gt.windows; ++w) {
      apt g = gt_load(gt, w, gt_next_digit(u, gt.bits));
      acc = jpt29_add_affine(acc, fe29_from_words(g.x.v), fe29_from_words(g.y.v));
    }
    {   // the last addition apart: whether Z was 0 before it is what the verdict code needs to know
      apt g = gt_load(gt, gt.windows - 1, gt_next_digit(u, gt.bits));
      if constexpr (ECDSA) final_only = !fe29_is_zero(acc.z);
      acc = jpt29_add_affine(acc, fe29_from_words(g.x.v), fe29_from_words(g.y.v));
    }
  }

  // ---- verdict ----
  uint8_t verdict = 0;
  // (MODE_RECOVER / MODE_POINT: the 65-byte records start as zeros - one fill of the output array by the caller; the loop of
  // 65 single-byte stores per lane that used to stand here cost the recovery ladder a tenth of its time)
  // Z = 0: infinity, or an exceptional case of the incomplete formulas somewhere on the way.  Where the zero first appears
  // in the FINAL addition of two finite points (Z3 = Z1 Z2 H = 0: equal x) the answer is at hand.  With H = 0 the mixed
  // addition leaves X3 = I^2, I = Y1 - S2 (jacobian29.h), so X3 != 0 says OPPOSITE points: R is the identity and verify
  // rejects it (ecdsa.go:450).  That is what anyone who owns a key gets with r = -e/d in every lane, whatever the digests
  // (the signature need not be valid), and it used to send the whole batch through the complete-formula kernel: 3.4 x a
  // normal step; now the lane is done.  X3 = 0 says EQUAL points (r = e/d): R is twice the last addend - left to the
  // worklist kernel with a tag (WL_DOUBLE_GEN: 2 u1 G in the grouped flows, WL_DOUBLE_LAST: twice the last generator-table
  // entry in the plain one; a twelfth of a full verification or less), since the keyed ladder has no registers to spare.
  // Zeros from INSIDE the ladder or the generator part (and u1 = 0: a digest that is 0 mod n) go to the worklist as before.
  bool undecided = ok && fe29_is_zero(acc.z), is_identity = false;
  uint32_t wl_tag = 0;
  if constexpr (ECDSA) {
    if (force_wl && ok) {                                // S2K_ECDSA_FORCE_WORKLIST (diagnostic)
      undecided = true;
      final_only = false;
    }
  }
  if constexpr (ECDSA) {
    if (undecided && final_only) {
      if (!fe29_is_zero(acc.x)) {
        undecided = false;
        is_identity = true;                              // P - P
      } else if (n < WL_TAG_LIMIT) {
        wl_tag = GROUPED ? WL_DOUBLE_GEN : WL_DOUBLE_LAST;   // P + P: R = 2 u1 G, or twice the last table entry
      }
    }
  }
  if (ok) {
    if (undecided) {
      // infinity or an exceptional case inside the ladder: the complete kernel decides
      uint32_t pos = atomicAdd(wl_count, 1u);
      wl[pos] = (uint32_t)sig | wl_tag;
    } else if (is_identity) {
      verdict = 0;                                      // R = infinity (ecdsa.go:450)
    } else if constexpr (!ECDSA) {
      // affine epilogue (key bytes / even-y test) needs 1/Z: leave (X, Y, Z) in the SIGNATURE's fin
      // column (its own lane's when not grouped) and let k_affine_finish share one inversion between 16
      fq_store(fin, stride, sig, 0, acc.x);
      fq_store(fin, stride, sig, 1, acc.y);
      fq_store(fin, stride, sig, 2, acc.z);
      verdict = VERDICT_PENDING;
    } else {
      // x(R) mod n == r  (ecdsa.go:450-465)
      uint32_t rw[8];
      load_be32(rw, rsig + sig * 32);
      fe29 zz = fe29_sqr(acc.z);
      bool match = fe29_eq(acc.x, fe29_mul(fe29_from_words(rw), zz));
      if (u256_lt(rw, FE_P_MINUS_N)) {
        uint32_t r2[8];
        u256_add(r2, rw, SC_N);
        match = match || fe29_eq(acc.x, fe29_mul(fe29_from_words(r2), zz));
      }
      verdict = match ? 1 : 0;
    }
  }
  out[sig] = verdict;
  if (stamp && threadIdx.x == 0) {
    uint64_t* c = clk + (blockIdx.x == 0 ? 0 : 4);
    c[0] = t0c;
    c[1] = __builtin_readcyclecounter();
    c[2] = t0w;
    c[3] = __builtin_amdgcn_s_memrealtime();
  }
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

// SchnorrPublicKey.Verify (schnorr.go:221-253) with complete formulas
S2K_DEV uint8_t schnorr_verify_complete(size_t idx, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
                                        const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs,
                                        uint32_t msg_len, gt_view gt, uint32_t* __restrict__ qt,
                                        size_t stride) {
  sc s, e;
  bool ok = schnorr_parse(idx, pk, sig, msgs, offs, msg_len, s, e);
  apt P;
  load_be32(P.x.v, pk + idx * 32);
  ok = ok && fe_is_canonical_raw(P.x.v);
  fe y;
  bool has = fe_sqrt(y, fe_curve_rhs(P.x));
  ok = ok && has;
  if (!ok) {
    P.x = fe_from_limbs(FE_GX);
    y = fe_from_limbs(FE_GY);
  }
  y = fe_normalize(y);
  P.y = fe_normalize(fe_select((y.v[0] & 1u) != 0, y, fe_neg(y)));
  pt R = pt_add_complete(pt_base_mul(gt, s.v), pt_mul_glv(sc_neg(e), P, qt, stride, idx));
  apt a;
  bool finite = pt_to_affine(a, R);
  uint32_t r_le[8];
  load_be32(r_le, sig + idx * 64);
  return (ok && finite && (a.y.v[0] & 1u) == 0 && u256_eq(a.x.v, r_le)) ? 1 : 0;
}

__global__ void __launch_bounds__(256)
k_schnorr_fallback(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, uint32_t all_n,
                   const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msgs,
                   const uint64_t* __restrict__ offs, uint32_t msg_len, uint8_t* __restrict__ out,
                   gt_view gt, uint32_t* __restrict__ qt, size_t stride) {
  // all_n != 0: diagnostic mode, every signature through the complete path
  uint32_t count = all_n ? all_n : *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    size_t idx = all_n ? w : wl[w];
    out[idx] = schnorr_verify_complete(idx, pk, sig, msgs, offs, msg_len, gt, qt, stride);
  }
}

// RecoverPublicKey (ecdsa.go:244-282) for one item with complete formulas
S2K_DEV uint8_t recover_complete(size_t idx, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig,
                                 const uint8_t* __restrict__ ssig, const uint8_t* __restrict__ recid,
                                 uint8_t* __restrict__ out_pts, gt_view gt,
                                 uint32_t* __restrict__ qt, size_t stride) {
  sc r, s;
  uint32_t e_raw[8];
  load_be32(r.v, rsig + idx * 32);
  load_be32(s.v, ssig + idx * 32);
  load_be32(e_raw, dig + idx * 32);
  uint32_t rid = recid[idx];
  bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && sc_is_canonical_raw(s.v) && !sc_is_zero(s) && rid < 4 &&
            (!(rid & 2u) || u256_lt(r.v, FE_P_MINUS_N));
  apt R;
#pragma unroll
  for (int i = 0; i < 8; ++i) R.x.v[i] = r.v[i];
  if (ok && (rid & 2u)) u256_add(R.x.v, R.x.v, SC_N);
  fe y;
  bool has = fe_sqrt(y, fe_curve_rhs(R.x));
  ok = ok && has;
  if (!ok) {
    R.x = fe_from_limbs(FE_GX);
    y = fe_from_limbs(FE_GY);
  }
  y = fe_normalize(y);
  R.y = fe_normalize(fe_select(((y.v[0] & 1u) != 0) != ((rid & 1u) != 0), y, fe_neg(y)));
  sc e = sc_reduce_once(e_raw);
  sc r_inv_m = sc_mont_inv(sc_to_mont(r));
  sc u1 = sc_montmul(sc_neg(e), r_inv_m), u2 = sc_montmul(s, r_inv_m);
  pt Q = pt_add_complete(pt_base_mul(gt, u1.v), pt_mul_glv(u2, R, qt, stride, idx));
  uint8_t* rec = out_pts + idx * 65;
  apt a;
  bool finite = pt_to_affine(a, Q);              // identity: NewPublicKeyFromPoint fails (secec.go:206-209)
  if (!(ok && finite)) {
    for (int i = 0; i < 65; ++i) rec[i] = 0;
    return 0;
  }
  rec[0] = 0x04;
  store_be32_unaligned(rec + 1, a.x.v);
  store_be32_unaligned(rec + 33, a.y.v);
  return 1;
}

__global__ void __launch_bounds__(256)
k_recover_fallback(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, uint32_t all_n,
                   const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig,
                   const uint8_t* __restrict__ recid, uint8_t* __restrict__ ok_out, uint8_t* __restrict__ out_pts,
                   gt_view gt, uint32_t* __restrict__ qt, size_t stride) {
  uint32_t count = all_n ? all_n : *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    size_t idx = all_n ? w : wl[w];
    ok_out[idx] = recover_complete(idx, dig, rsig, ssig, recid, out_pts, gt, qt, stride);
  }
}

// x/Z, y/Z of a projective 9x29 point (canonical words); false for the identity
S2K_DEV bool p29_to_affine_words(uint32_t xw[8], uint32_t yw[8], const pt29& p) {
  if (fe29_is_zero(p.z)) return false;
  fe29 zi = fe29_inv_gcd(fe29_normalize_weak(p.z));
  fe29_to_words(xw, fe29_normalize(fe29_mul(p.x, zi)));
  fe29_to_words(yw, fe29_normalize(fe29_mul(p.y, zi)));
  return true;
}
// lift_x on the 9x29 field: y with the wanted parity for a canonical x (words), or false
S2K_DEV bool lift_x29(fe29& x, fe29& y, const uint32_t xw[8], bool want_odd) {
  x = fe29_from_words(xw);
  fe29 rhs = fe29_mul(fe29_sqr(x), x);
  rhs.n[0] += 7;
  if (!fe29_sqrt(y, rhs)) return false;
  y = fe29_normalize(y);
  y = fe29_select(((y.n[0] & 1u) != 0) != want_odd, y, fe29_normalize_weak(fe29_negate(y, 1)));
  return true;
}

// The worklists of the BIP-340 and recovery paths, same verifier core (9x29 complete formulas) as
// the ECDSA worklist; the reference-shaped 8x32 versions above stay for S2K_ECDSA_FORCE_COMPLETE.
__global__ void __launch_bounds__(256)
k_schnorr_worklist(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, const uint8_t* __restrict__ pk,
                   const uint8_t* __restrict__ sig, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs,
                   uint32_t msg_len, uint8_t* __restrict__ out, gt_view gt, uint32_t* __restrict__ qt,
                   size_t stride) {
  const uint32_t count = *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    const size_t idx = wl[w];
    sc s, e;
    bool ok = schnorr_parse(idx, pk, sig, msgs, offs, msg_len, s, e);
    uint32_t xw[8];
    load_be32(xw, pk + idx * 32);
    ok = ok && fe_is_canonical_raw(xw);
    if (!ok) {
#pragma unroll
      for (int i = 0; i < 8; ++i) xw[i] = FE_GX[i];
    }
    fe29 px, py;
    if (!lift_x29(px, py, xw, false)) {   // not an x-coordinate of the curve (NewSchnorrPublicKey, schnorr.go:257-275)
      ok = false;
      px = fe29_from_words(FE_GX);
      py = fe29_from_words(FE_GY);
    }
    pt29 R = dsm_complete29(s, sc_neg(e), px, py, gt, qt, stride, w);   // s*G - e*P (schnorr.go:244); table column = worklist position
    uint32_t rx[8], ry[8], r_le[8];
    bool finite = p29_to_affine_words(rx, ry, R);
    load_be32(r_le, sig + idx * 64);
    out[idx] = (ok && finite && (ry[0] & 1u) == 0 && u256_eq(rx, r_le)) ? 1 : 0;   // verifySchnorrSignatureR (:451-478)
  }
}

__global__ void __launch_bounds__(256)
k_recover_worklist(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, const uint8_t* __restrict__ dig,
                   const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig, const uint8_t* __restrict__ recid,
                   uint8_t* __restrict__ ok_out, uint8_t* __restrict__ out_pts, gt_view gt,
                   uint32_t* __restrict__ qt, size_t stride) {
  const uint32_t count = *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    const size_t idx = wl[w];
    sc r, s;
    uint32_t e_raw[8], xw[8];
    load_be32(r.v, rsig + idx * 32);
    load_be32(s.v, ssig + idx * 32);
    load_be32(e_raw, dig + idx * 32);
    const uint32_t rid = recid[idx];
    bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && sc_is_canonical_raw(s.v) && !sc_is_zero(s) && rid < 4 &&
              (!(rid & 2u) || u256_lt(r.v, FE_P_MINUS_N));   // RecoverPoint (point_s11n.go:245-282)
#pragma unroll
    for (int i = 0; i < 8; ++i) xw[i] = r.v[i];
    if (ok && (rid & 2u)) u256_add(xw, xw, SC_N);
    if (!ok) {
#pragma unroll
      for (int i = 0; i < 8; ++i) xw[i] = FE_GX[i];
      r = sc_zero();
      r.v[0] = 1;
    }
    fe29 px, py;
    if (!lift_x29(px, py, xw, (rid & 1u) != 0)) {
      ok = false;
      px = fe29_from_words(FE_GX);
      py = fe29_from_words(FE_GY);
    }
    sc e = sc_reduce_once(e_raw);
    sc26 r_inv_m = sc26_mont_inv(sc26_to_mont(sc26_from_sc(r)));
    sc u1 = sc26_to_sc(sc26_mm(sc26_from_sc(sc_neg(e)), r_inv_m)), u2 = sc26_to_sc(sc26_mm(sc26_from_sc(s), r_inv_m));
    pt29 Q = dsm_complete29(u1, u2, px, py, gt, qt, stride, idx);   // (-e/r) G + (s/r) R (ecdsa.go:244-282)
    uint32_t qxw[8], qyw[8];
    bool finite = p29_to_affine_words(qxw, qyw, Q);   // identity: NewPublicKeyFromPoint fails (secec.go:206-209)
    uint8_t* rec = out_pts + idx * 65;
    if (!(ok && finite)) {
      for (int i = 0; i < 65; ++i) rec[i] = 0;
      ok_out[idx] = 0;
    } else {
      rec[0] = 0x04;
      store_be32_unaligned(rec + 1, qxw);
      store_be32_unaligned(rec + 33, qyw);
      ok_out[idx] = 1;
    }
  }
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

// ALL: every item (S2K_IMPL_COMPLETE); otherwise the worklist.  u1 is always present (the host
// passes zeros for a plain scalar multiplication): the conditional form of this kernel
// (`if (u1)` around the generator part, `all_n ? w : wl[w]` for the index) was miscompiled by
// hipcc 7.2 -- per-lane garbage for half of the inputs, reproduced standalone in tools/dbg/ --
// so the kernel keeps to the shape of k_recover_fallback, which is not.
template <bool ALL>
__global__ void __launch_bounds__(256)
k_point_fallback(const uint32_t* __restrict__ wl_count, const uint32_t* __restrict__ wl, uint32_t n,
                 const uint8_t* __restrict__ u1, const uint8_t* __restrict__ u2, const uint8_t* __restrict__ pts65,
                 uint8_t* __restrict__ out65, gt_view gt, uint32_t* __restrict__ qt, size_t stride,
                 uint32_t* __restrict__ status) {
  uint32_t count;
  if constexpr (ALL) count = n; else count = *wl_count;
  for (uint32_t w = blockIdx.x * 256 + threadIdx.x; w < count; w += gridDim.x * 256) {
    size_t idx;
    if constexpr (ALL) idx = w; else idx = wl[w];
    const uint8_t* rec = pts65 + idx * 65;
    apt a;
    load_be32_unaligned(a.x.v, rec + 1);
    load_be32_unaligned(a.y.v, rec + 33);
    bool finite = rec[0] == 0x04 && fe_is_canonical_raw(a.x.v) && fe_is_canonical_raw(a.y.v) && apt_on_curve(a);
    if (!finite && rec[0] != 0x00) atomicOr(status, 1u);
    if (!finite) {   // keep the arithmetic on the curve; the term is masked below
      a.x = fe_from_limbs(FE_GX);
      a.y = fe_from_limbs(FE_GY);
    }
    uint32_t raw1[8], raw2[8];
    load_be32(raw1, u1 + idx * 32);
    load_be32(raw2, u2 + idx * 32);
    sc v1 = sc_reduce_once(raw1), v2 = sc_reduce_once(raw2);
    pt rq = pt_mul_glv(v2, a, qt, stride, idx);
    rq = pt_select(!finite, rq, pt_identity());
    pt res = pt_add_complete(pt_base_mul(gt, v1.v), rq);   // point_mul_glv.go:316
    uint8_t* o = out65 + idx * 65;
    apt r;
    if (!pt_to_affine(r, res)) {
      for (int j = 0; j < 65; ++j) o[j] = 0;
    } else {
      o[0] = 0x04;
      store_be32_unaligned(o + 1, r.x.v);
      store_be32_unaligned(o + 33, r.y.v);
    }
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// per-stage timing (s2k_ctx_profile): six events per call, around scalar preparation | grouping and
// per-key tables | ladder (keyed, or the general one when grouping is off) | general ladder over the
// ungrouped rest | complete-formula worklist
constexpr int PROF_EV = 6;
__attribute__((visibility("hidden"))) void prof_mark(s2k_ctx* ctx, hipStream_t st, int slot) {
  if (!ctx->prof_on || ctx->prof_used + PROF_EV > ctx->prof_cap) return;
  (void)hipEventRecord(ctx->prof_ev[ctx->prof_used + slot], st);
  if (slot == PROF_EV - 1) ctx->prof_used += PROF_EV;
}

// One launcher per kernel: it enqueues on the stream it is given and does nothing else (error checks, events and profiling
// marks stay with the flows).  `ctx` gives the call's generator table (gt_call) and the worklist kernels' grid.
// launch_scalar_prep: signatures [first, first + count) on `lanes` lanes (the planes are linear in the signature index: a piece
// is the same kernel on shifted pointers); launch_ladder: the only place that names an instantiation of k_verify_fast.
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
static void launch_ecdsa_verify(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pub, const uint8_t* dig,
                                const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_ecdsa_verify<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, pub, dig, r, s, flags, out, ctx->gt_call, w.qt, w.stride);
}
__attribute__((visibility("hidden"))) void launch_verify_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pub, const uint8_t* dig,
                                   const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_verify_fallback<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, pub, dig, r, s, flags, out, ctx->gt_call, w.qt, w.stride);
}
__attribute__((visibility("hidden"))) void launch_verify_fallback_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* keys, const uint32_t* kidx,
                                          const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_verify_fallback_keyset<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, keys, kidx, dig, r, s, flags, out, ctx->gt_call, w.qt,
                                                                    w.stride);
}
__attribute__((visibility("hidden"))) void launch_schnorr_prep(hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs,
                                const uint64_t* offs, uint32_t msg_len) {
  k_schnorr_prep<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, pk, sig, msgs, offs, msg_len, w.prep, w.stride);
}
static void launch_schnorr_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig,
                                    const uint8_t* msgs, const uint64_t* offs, uint32_t msg_len, uint8_t* out) {
  k_schnorr_fallback<<<blocks_for(n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, pk, sig, msgs, offs, msg_len, out, ctx->gt_call, w.qt,
                                                    w.stride);
}
__attribute__((visibility("hidden"))) void launch_schnorr_worklist(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig,
                                    const uint8_t* msgs, const uint64_t* offs, uint32_t msg_len, uint8_t* out) {
  k_schnorr_worklist<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, pk, sig, msgs, offs, msg_len, out, ctx->gt_call, w.qt,
                                                              w.stride);
}
static void launch_recover_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* dig, const uint8_t* r,
                                    const uint8_t* s, const uint8_t* recid, uint8_t* ok, uint8_t* pub65) {
  k_recover_fallback<<<blocks_for(n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, dig, r, s, recid, ok, pub65, ctx->gt_call, w.qt, w.stride);
}
static void launch_recover_worklist(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* dig, const uint8_t* r,
                                    const uint8_t* s, const uint8_t* recid, uint8_t* ok, uint8_t* pub65) {
  k_recover_worklist<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, dig, r, s, recid, ok, pub65, ctx->gt_call, w.qt, w.stride);
}
static void launch_hot_prep(hipStream_t st, size_t n, const lane_ws& w, const uint8_t* u1, const uint8_t* u2, const uint8_t* pts65, uint8_t* pub64,
                            uint32_t* status) {
  k_hot_prep<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, u1, u2, pts65, pub64, w.prep, w.stride, w.wl_count, w.wl, status);
}
static void launch_point_fallback(const s2k_ctx* ctx, hipStream_t st, bool all, size_t n, const lane_ws& w, const uint8_t* u1, const uint8_t* u2,
                                  const uint8_t* pts65, uint8_t* out65, uint32_t* status) {
  if (all)
    k_point_fallback<true><<<blocks_for(n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, u1, u2, pts65, out65, ctx->gt_call, w.qt, w.stride,
                                                          status);
  else
    k_point_fallback<false><<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, u1, u2, pts65, out65, ctx->gt_call, w.qt,
                                                                     w.stride, status);
}

// Front end of the grouped flows (ECDSA and BIP-340 verification): everything up to the ladders.
// Caller's stream: grouping by key (k_key_insert / k_key_alloc / k_key_place), then the per-key tables.
// Second stream: the scalar preparation (`launch_prep`), then the generator part u1*G in two pieces.  These
// have nothing to do with the keys and the grouping / table kernels are short of work for the multipliers
// on their own (the doubling chain of the tables is one lane per KEY, the scaling pass is memory bound).
// The first piece of the generator part runs beside the chain, the second beside k_key_finish (its event sits in
// front of that kernel; between k_key_odd and k_key_cofactors where the three older kernels build the tables).  The
// share of the first piece (S2K_GP_FIRST_PERCENT, 60) is flat between 30 and 100 and costs 0.3 ms at 0
// (profiles/r07_key_finish_ab.txt).  Returns with the caller's stream waiting for the second.
// Stage times (s2k_ctx_profile_read_stages): [0] grouping, [1] tables and whatever is left of the second
// stream's work.
// S2K_KEYS_ADAPTIVE (engine_internal.h: kga_*): takes in the notes that have arrived, decides whether this call looks for
// repeated keys, and if it does, where its k_key_counts leaves its note.  No device call that waits.
static bool kg_adaptive_decide(s2k_ctx* ctx) {
  s2k_ctx* own = ctx->parent ? ctx->parent : ctx;
  if (!own->kga_note) {
    void* p = nullptr;
    if (hipHostMalloc(&p, KG_ADAPT_SLOTS * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return true;                                     // no note, no learning: S2K_KEYS_AUTO
    }
    memset(p, 0, KG_ADAPT_SLOTS * sizeof(unsigned long long));
    own->kga_note = (unsigned long long*)p;
  }
  for (;;) {                                           // notes in the order of their numbers; a slot overwritten by a later call: that one
    unsigned long long next = 0;
    for (uint32_t i = 0; i < KG_ADAPT_SLOTS; ++i) {
      const unsigned long long v = __atomic_load_n(&own->kga_note[i], __ATOMIC_ACQUIRE);
      const uint32_t sq = (uint32_t)(v >> 32);
      if (v && (int32_t)(sq - own->kga_seen) > 0 && (!next || (int32_t)(sq - (uint32_t)(next >> 32)) < 0)) next = v;
    }
    if (!next) break;
    own->kga_seen = (uint32_t)(next >> 32);
    ++own->kga_observed;
    if ((uint32_t)next == 0) {
      ++own->kga_miss_streak;
    } else {
      own->kga_miss_streak = 0;
      own->kga_skip_left = 0;
      own->kga_skipping = false;
    }
  }
  if (own->kga_miss_streak >= KG_ADAPT_MISSES) {
    if (!own->kga_skipping) {
      own->kga_skipping = true;
      own->kga_skip_left = KG_ADAPT_SKIP;
    }
    if (own->kga_skip_left) {
      --own->kga_skip_left;
      ++own->kga_skipped;
      return false;
    }
    own->kga_skip_left = KG_ADAPT_SKIP;                // this call looks again; the next ones do not, unless it finds something
    ++own->kga_probes;
  } else {
    own->kga_skipping = false;
  }
  if (++own->kga_seq == 0) own->kga_seq = 1;           // (0 marks an empty slot)
  ctx->kg_note_seq = own->kga_seq;
  ctx->kg_note_dst = own->kga_note + own->kga_seq % KG_ADAPT_SLOTS;
  return true;
}

template <class PrepFn>
static int grouped_front_forked(s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* d_keys, int key_bytes, const lane_ws& w,
                                PrepFn launch_prep, key_groups* kg, bool gp_in_prep) {
  // One stream (a child context of submit / wait): the grouping and the tables first - they need the keys only, which
  // arrive first -, then the preparation and the generator part; other tickets' kernels fill the machine meanwhile.
  const bool one_stream = ctx->s_aux == st;
  // gp_in_prep: the caller's launch_prep has enqueued the generator part as well (piecewise, as its inputs arrive)
  const uint32_t n_first = (gp_in_prep || one_stream) ? (gp_in_prep ? (uint32_t)n : 0u)
                                                      : (uint32_t)((n * (size_t)ctx->gp_first_percent / 100) & ~(size_t)255);
  if (!one_stream) {
    launch_prep(ctx->s_aux);
    HIP_TRY(ctx, hipGetLastError());
    if (n_first && !gp_in_prep) {
      launch_generator_part(ctx, ctx->s_aux, w, 0u, n_first);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  int rc = s2k_internal_key_group(ctx, n, d_keys, key_bytes, st, kg);
  if (rc) return rc;
  kg->gp = w.gp;
  kg->part = 0;
  kg->nparts = ctx->kg_parts;
  prof_mark(ctx, st, 1);
  rc = s2k_internal_key_chains(ctx, d_keys, st, kg);
  if (rc) return rc;
  // Two-part flow (S2K_KEYED_PARTS=2, off by default): the tables of the first half of the keys here; those
  // of the second half on a third stream, started when these are done, i.e. beside the first half's ladder.
  // Measured: the tables' share of the step shrinks by 0.3 ms and the ladders grow by 0.36 (2^16 keys: 5.27-5.30
  // against 5.22 ms; 2^17 keys: 6.33 against 6.12-6.21) - the table kernels' traffic costs the ladder more
  // than their idle multipliers give it.
  rc = s2k_internal_key_tables(ctx, st, kg, 0, kg->nparts, ctx->ev_mid);
  if (rc) return rc;
  if (kg->nparts > 1) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_part0, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux2, ctx->ev_part0, 0));
    rc = s2k_internal_key_tables(ctx, ctx->s_aux2, kg, 1, kg->nparts, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_part1, ctx->s_aux2));
  }
  if (one_stream) {
    launch_prep(st);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux, ctx->ev_mid, 0));
  }
  if (n_first < n) {
    launch_generator_part(ctx, ctx->s_aux, w, n_first, (uint32_t)n);
    HIP_TRY(ctx, hipGetLastError());
  }
  return S2K_OK;
}
template <class PrepFn>
static int grouped_front(s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* d_keys, int key_bytes, const lane_ws& w,
                         PrepFn launch_prep, key_groups* kg, bool gp_in_prep = false) {
  int rc = ctx_aux_streams(ctx);
  if (rc) return rc;
  // the buffers the grouping needs are reserved BEFORE the fork: growing one is a device-wide synchronisation
  // (hipFree), which must not meet work of this call in flight on the second stream
  rc = s2k_internal_key_reserve(ctx, n, key_bytes);
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux, ctx->ev_fork, 0));
  rc = grouped_front_forked(ctx, st, n, d_keys, key_bytes, w, launch_prep, kg, gp_in_prep);
  // error or not, the caller's stream waits for the second one again, and the context's next call for this one: an
  // error return leaves nothing of this call in flight behind the context's back
  ctx_aux_join(ctx, st);
  if (kg->nparts > 1 && rc == S2K_OK) { /* (ev_part1 is waited for by the caller, before the second ladder) */ }
  if (rc) {
    if (ctx->s_aux2) {
      (void)hipEventRecord(ctx->ev_part1, ctx->s_aux2);
      (void)hipStreamWaitEvent(st, ctx->ev_part1, 0);
    }
    (void)ctx_leave(ctx, st);
  }
  return rc;
}

s2k_phase_locks& s2k_internal_phase(int device) {
  static s2k_phase_locks locks[64];
  return locks[device & 63];
}

extern "C" {

const char* s2k_version(void) { return "secp256k1_voi_amd 0.4 (gfx950)"; }
#define S2K_STR2(x) #x
#define S2K_STR(x) S2K_STR2(x)
#ifndef S2K_BUILD_FLAGS
#define S2K_BUILD_FLAGS ""
#endif
const char* s2k_build_config(void) {
  return "GT_BITS=" S2K_STR(S2K_GT_BITS) " GT_BITS_FIRST=" S2K_STR(S2K_GT_BITS_FIRST) " PREP_M=" S2K_STR(S2K_PREP_M)
         " QT_PACK=" S2K_STR(S2K_QT_PACK) " FAST_WAVES=" S2K_STR(S2K_FAST_WAVES) " STRIDE_PAD=" S2K_STR(S2K_STRIDE_PAD)
         " ROW_MAX=" S2K_STR(S2K_ROW_MAX_DEFAULT) " QUAD_MAX=" S2K_STR(S2K_QUAD_MAX_DEFAULT) " COMB_LEAD=" S2K_STR(S2K_COMB_LEAD_DEFAULT)
         " flags=[" S2K_BUILD_FLAGS "]";
}
const char* s2k_last_error(const s2k_ctx* ctx) { return ctx ? ctx->err : g_err; }
int s2k_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}
// "0000:05:00.0" of a device (hipDeviceGetPCIBusId): what topology.cpp looks up in sysfs
int s2k_device_pci_bus_id(int device, char* out, size_t len) {
  if (!out || len < 13) return S2K_ERR_ARG;
  out[0] = 0;
  if (hipDeviceGetPCIBusId(out, (int)len, device) != hipSuccess) {
    (void)hipGetLastError();
    out[0] = 0;
    return S2K_ERR_NO_DEVICE;
  }
  return S2K_OK;
}

// workspace (32-bit words per lane, lane stride = n rounded up to 64):
//   [0,256)    per-lane point table of the fast path: 8 entries x 8 quads (tb_*); the complete path
//              uses the first 192 words for its projective table
//   [256,304)  four scratch field elements ("fin": X, Y, Z for k_affine_finish; Z_7*C / prefix products)
//   then       17 words of scalar-prep output, 36 words for the generator part (grouped flow).  The prep kernel's own scratch (prefix products and
//              s in Montgomery form, 10 words each) borrows the start of the table region,
//              which is only written after the prep kernel has finished.
//   then       worklist: 1 counter + n indices
constexpr size_t WS_QT = 0, WS_FIN = TBL_WORDS, WS_PREP = TBL_WORDS + FIN_WORDS, WS_PREF = WS_QT, WS_SMONT = WS_QT + 10,
                 WS_GP = WS_PREP + PREP_WORDS, WS_LANE_WORDS = WS_GP + 3 * FQT_FE_WORDS;
static_assert(TBL_WORDS >= QT_WORDS, "the complete path's table must fit in the fast path's region");
}  // extern "C"
__attribute__((visibility("hidden"))) lane_ws lane_ws_of(const s2k_ctx* ctx, size_t n) {
  const size_t stride = lane_stride(n);
  uint32_t* ws = (uint32_t*)ctx->ws;
  lane_ws w;
  w.qt = ws + WS_QT * stride;
  w.fin = ws + WS_FIN * stride;
  w.prep = ws + WS_PREP * stride;
  w.gp = ws + WS_GP * stride;
  w.pref = ws + WS_PREF * stride;
  w.smont = ws + WS_SMONT * stride;
  w.wl_count = ws + WS_LANE_WORDS * stride;
  w.wl = w.wl_count + 64;
  w.stride = stride;
  return w;
}
extern "C" {

size_t s2k_ecdsa_workspace_bytes(size_t n) {
  return (lane_stride(n) * WS_LANE_WORDS + 64 + lane_stride(n)) * sizeof(uint32_t);
}
size_t s2k_ctx_device_bytes(const s2k_ctx* ctx, size_t n) {
  if (!ctx) return 0;
  size_t total = s2k_ecdsa_workspace_bytes(n);
  {
    uint64_t info[4] = {0, 0, 0, 0};
    (void)s2k_ctx_gt_info(const_cast<s2k_ctx*>(ctx), info);
    total += (size_t)info[3] + (info[2] ? gt_bytes_of((int)info[1]) : 0);   // the tables held, and the one being built
  }
  if (ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH) total += s2k_internal_key_bytes(ctx, n);
  return total;
}

// (shared with ops.hip; not part of the ABI)
__attribute__((visibility("hidden"))) int s2k_internal_ensure_ws(s2k_ctx* ctx, size_t n) {
  size_t need = s2k_ecdsa_workspace_bytes(n);
  if (need <= ctx->ws_bytes) return S2K_OK;
  if (ctx->ws) {
    HIP_TRY(ctx, hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    ctx->last_wl_count = nullptr;   // pointed into the old workspace (s2k_ctx_key_grouping_stats)
  }
  HIP_TRY(ctx, hipMalloc(&ctx->ws, need));
  ctx->ws_bytes = need;
  return S2K_OK;
}

namespace {
std::atomic<size_t> g_keyset_budget{0};           // s2k_set_table_memory_budgets: what counts as free for a key set's joint tables (0: what is free)
}  // namespace
// (pointset.hip: a point set's tables count against the same cap as a key set's joint tables)
__attribute__((visibility("hidden"))) size_t s2k_internal_keyset_budget() { return g_keyset_budget.load(); }

extern "C" {
// Caps on the two other table kinds, per process (0 = none): what s2k_keyset_create_ex treats as free memory when it chooses or
// checks a joint-table layout, and the largest per-key table buffer a verification call may allocate (larger requests are
// treated as failed allocations: the table cap halves, below 1024 tables the batch is verified without tables).  These replace
// the S2K_TEST_* environment variables of round 4 (no ambient test hooks in allocation paths).
void s2k_set_table_memory_budgets(size_t keyset_free_bytes, size_t key_table_bytes) {
  g_keyset_budget.store(keyset_free_bytes);
  s2k_internal_key_table_limit().store(key_table_bytes);
}
}  // extern "C"

int s2k_ctx_create(int device_index, s2k_ctx** out) { return s2k_ctx_create_ex(device_index, 0, 0, out); }

// gt_bits: 0 = automatic (above); 16 .. 26 = exactly that window width for this context's generator tables, built before the
// call returns.  flags: S2K_CTX_WAIT_TABLES = return only when the background build has ended (a context that must run at
// full speed from its first call: benchmarks).
int s2k_ctx_create_ex(int device_index, int gt_bits, uint32_t flags, s2k_ctx** out) {
  if (!out) return fail(nullptr, S2K_ERR_ARG, "s2k_ctx_create: out is NULL");
  *out = nullptr;
  if (gt_bits != 0 && (gt_bits < 16 || gt_bits > GT_BITS_MAX)) return fail(nullptr, S2K_ERR_ARG, "generator window width %d: 0 (automatic) or 16 .. %d", gt_bits, GT_BITS_MAX);
  if (flags & ~(uint32_t)S2K_CTX_WAIT_TABLES) return fail(nullptr, S2K_ERR_ARG, "unknown context flags");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(nullptr, S2K_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
  if (device_index < 0 || device_index >= count)
    return fail(nullptr, S2K_ERR_ARG, "device index %d out of range (0..%d)", device_index, count - 1);
  s2k_ctx* ctx = new (std::nothrow) s2k_ctx();
  if (!ctx) return fail(nullptr, S2K_ERR_NOMEM, "out of host memory");
  ctx->device = device_index;
  {
    static std::atomic<uint64_t> next_generation{1};
    ctx->generation = next_generation.fetch_add(1);
  }
  if (getrandom(&ctx->kg_seed, sizeof ctx->kg_seed, 0) != (ssize_t)sizeof ctx->kg_seed) ctx->kg_seed = 0x5ec9u;   // hash seed of the key grouping
  if (const char* v = getenv("S2K_KEYED_PARTS")) {        // measurement knob: 2 = the two-part flow (grouped_front)
    int np = atoi(v);
    if (np == 1 || np == 2) ctx->kg_parts = (uint32_t)np;
  }
  if (const char* v = getenv("S2K_KEYED_LADDER")) {       // "window": the ECDSA and BIP-340 calls of this context build 16-bit chunk tables (s2k_ctx_set_keyed_ladder)
    if (!strcmp(v, "window")) ctx->kt_comb = false;
  }
  if (const char* v = getenv("S2K_GP_FIRST_PERCENT")) {   // measurement knob (tools/keyed_probe.py)
    int pc = atoi(v);
    if (pc >= 0 && pc <= 100) ctx->gp_first_percent = (uint32_t)pc;
  }
  hipError_t e = hipSetDevice(device_index);
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device_index);
  if (e == hipSuccess) ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->clk, 64);
  if (e == hipSuccess) e = hipMemset(ctx->clk, 0, 64);
  if (e == hipSuccess) {
    e = s2k_internal_gt_acquire(device_index, gt_bits);
    if (e == hipSuccess) {
      ctx->gt_held = true;
      ctx->gt_fixed = gt_bits;
    } else if (e == hipErrorOutOfMemory) {
      (void)fail(nullptr, S2K_ERR_NOMEM, "context creation failed: no device memory for the %d-bit generator tables (%.1f GiB)",
                 gt_bits ? gt_bits : GT_BITS_FIRST, gt_bytes_of(gt_bits ? gt_bits : GT_BITS_FIRST) / 1073741824.0);
    }
  }
  if (e != hipSuccess) {
    int rc = e == hipErrorOutOfMemory ? S2K_ERR_NOMEM : fail(nullptr, S2K_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
    if (ctx->clk) (void)hipFree(ctx->clk);
    if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
    delete ctx;
    return rc;
  }
  if (flags & S2K_CTX_WAIT_TABLES) (void)s2k_ctx_gt_wait(ctx);
  *out = ctx;
  return S2K_OK;
}

void s2k_ctx_destroy(s2k_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (s2k_ctx::pipe_slot& sl : ctx->pipe) {          // batches still in flight are waited for (their verdicts are delivered)
    if (sl.ctx) {
      (void)s2k_internal_pipe_retire(ctx, sl);
      s2k_ctx_destroy(sl.ctx);
      sl.ctx = nullptr;
    }
    if (sl.h_valid) (void)hipHostFree(sl.h_valid);
    sl.h_valid = nullptr;
    if (sl.done) (void)hipEventDestroy(sl.done);
    sl.done = nullptr;
    for (hipEvent_t* e : {&sl.t_begin, &sl.t_copied, &sl.t_end}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  }
  if (ctx->kga_note) {                                // (a kernel still in flight may hold the address)
    (void)hipDeviceSynchronize();
    (void)hipHostFree(ctx->kga_note);
  }
  if (ctx->gt_held) s2k_internal_gt_release(ctx->device);
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->msm_ws) (void)hipFree(ctx->msm_ws);
  if (ctx->seg_ws) (void)hipFree(ctx->seg_ws);
  if (ctx->seg_host) (void)hipHostFree(ctx->seg_host);
  if (ctx->h2c_dev) (void)hipFree(ctx->h2c_dev);
  if (ctx->h2c_host) (void)hipHostFree(ctx->h2c_host);
  if (ctx->rlc_save) (void)hipFree(ctx->rlc_save);
  if (ctx->msg_digest) (void)hipFree(ctx->msg_digest);
  if (ctx->io) (void)hipFree(ctx->io);
  if (ctx->h_small) (void)hipHostFree(ctx->h_small);
  if (ctx->clk) (void)hipFree(ctx->clk);
  if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
  if (ctx->s_aux && !ctx->streams_shared) (void)hipStreamDestroy(ctx->s_aux);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ev_mid) (void)hipEventDestroy(ctx->ev_mid);
  for (hipEvent_t& e : ctx->ev_arrival)
    if (e) (void)hipEventDestroy(e);
  if (ctx->ev_part0) (void)hipEventDestroy(ctx->ev_part0);
  if (ctx->ev_part1) (void)hipEventDestroy(ctx->ev_part1);
  if (ctx->s_aux2) (void)hipStreamDestroy(ctx->s_aux2);
  if (ctx->s_msm_tail) (void)hipStreamDestroy(ctx->s_msm_tail);
  if (ctx->kg) (void)hipFree(ctx->kg);
  if (ctx->ktab) (void)hipFree(ctx->ktab);
  if (ctx->xkeys) (void)hipFree(ctx->xkeys);
  if (ctx->ks_found) (void)hipFree(ctx->ks_found);
  if (ctx->ek_ctr) (void)hipFree(ctx->ek_ctr);
  for (size_t i = 0; i < ctx->prof_cap; ++i) (void)hipEventDestroy(ctx->prof_ev[i]);
  for (size_t i = 0; i < ctx->msm_prof_cap; ++i) (void)hipEventDestroy(ctx->msm_prof_ev[i]);
  delete[] ctx->msm_prof_ev;
  delete[] ctx->prof_ev;
  for (hipEvent_t e : ctx->ev_copied)
    if (e) (void)hipEventDestroy(e);
  if (ctx->lane1_comp) (void)hipStreamDestroy(ctx->lane1_comp);
  if (ctx->lane1_aux) (void)hipStreamDestroy(ctx->lane1_aux);
  if (ctx->s_copy && !ctx->streams_shared) (void)hipStreamDestroy(ctx->s_copy);
  if (ctx->s_comp && !ctx->streams_shared) (void)hipStreamDestroy(ctx->s_comp);
  delete ctx;
}

int s2k_ctx_profile(s2k_ctx* ctx, int enable) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (enable && !ctx->prof_ev) {
    const size_t cap = PROF_EV * 1024;   // 1024 verification calls between two reads
    ctx->prof_ev = new (std::nothrow) hipEvent_t[cap];
    if (!ctx->prof_ev) return fail(ctx, S2K_ERR_NOMEM, "out of host memory");
    for (size_t i = 0; i < cap; ++i) {
      hipError_t e = hipEventCreate(&ctx->prof_ev[i]);
      if (e != hipSuccess) {
        for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(ctx->prof_ev[j]);
        delete[] ctx->prof_ev;
        ctx->prof_ev = nullptr;
        return fail(ctx, S2K_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
      }
    }
    ctx->prof_cap = cap;
  }
  ctx->prof_on = enable != 0;
  ctx->prof_used = 0;
  return S2K_OK;
}

int s2k_ctx_profile_read_stages(s2k_ctx* ctx, double* ms_sum5, double* ms_fast_each, size_t cap, size_t* calls,
                                double* shader_mhz) {
  if (!ctx || !ms_sum5 || !calls) return fail(ctx, S2K_ERR_ARG, "null argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  for (int j = 0; j < PROF_EV - 1; ++j) ms_sum5[j] = 0.0;
  const size_t k = ctx->prof_used / PROF_EV;
  for (size_t i = 0; i < k; ++i) {
    for (int j = 0; j < PROF_EV - 1; ++j) {
      float ms = 0.f;
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->prof_ev[PROF_EV * i + j], ctx->prof_ev[PROF_EV * i + j + 1]));
      ms_sum5[j] += ms;
      if (j == 2 && ms_fast_each && i < cap) ms_fast_each[i] = ms;
    }
  }
  *calls = k;
  ctx->prof_used = 0;
  if (shader_mhz) {   // [0]: first wave of the last ladder launch, [1]: a wave of its final round
    uint64_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int wall_khz = 0;
    HIP_TRY(ctx, hipMemcpy(h, ctx->clk, sizeof h, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device));
    for (int j = 0; j < 2; ++j) {
      const uint64_t* c = h + 4 * j;
      shader_mhz[j] = (c[3] > c[2] && wall_khz > 0) ? (double)(c[1] - c[0]) / (double)(c[3] - c[2]) * (wall_khz * 1e-3) : 0.0;
    }
  }
  return S2K_OK;
}

// the three-stage view: preparation (with grouping and tables) | ladder | everything after it
int s2k_ctx_profile_read(s2k_ctx* ctx, double* ms_sum3, double* ms_fast_each, size_t cap, size_t* calls,
                         double* shader_mhz) {
  if (!ctx || !ms_sum3 || !calls) return fail(ctx, S2K_ERR_ARG, "null argument");
  double s5[5];
  int rc = s2k_ctx_profile_read_stages(ctx, s5, ms_fast_each, cap, calls, shader_mhz);
  if (rc) return rc;
  ms_sum3[0] = s5[0] + s5[1];
  ms_sum3[1] = s5[2];
  ms_sum3[2] = s5[3] + s5[4];
  return S2K_OK;
}

// `arrivals` (optional): d_dig / d_r / d_s become valid piece by piece - signatures [lo[c], lo[c] + cnt[c]) after event
// ev[c]; the keys (d_pub) are valid in stream order.  The host-buffer entry point copies the keys first and lets the
// grouping and the per-key tables - which need nothing else - start while the rest of the batch is still crossing PCIe;
// the scalar preparation and the generator part of a piece follow its arrival on the second stream.
struct sig_arrivals {
  int count;
  size_t lo[8], cnt[8];
  hipEvent_t ev[8];
};
static int verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r, const void* d_s,
                               uint32_t flags, void* d_valid, void* hip_stream, const sig_arrivals* arrivals);
int s2k_ecdsa_verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r,
                                  const void* d_s, uint32_t flags, void* d_valid, void* hip_stream) {
  return verify_batch_device(ctx, n, d_pub, d_dig, d_r, d_s, flags, d_valid, hip_stream, nullptr);
}
static int verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r, const void* d_s,
                               uint32_t flags, void* d_valid, void* hip_stream, const sig_arrivals* arrivals) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_pub || !d_dig || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  const lane_ws w = lane_ws_of(ctx, n);
  const uint8_t *pub = (const uint8_t*)d_pub, *dig = (const uint8_t*)d_dig, *r = (const uint8_t*)d_r, *s = (const uint8_t*)d_s;
  uint8_t* valid = (uint8_t*)d_valid;
  ctx->kg_counters = nullptr;
  ctx->last_wl_count = nullptr;
  ctx->kt_last = -1;
  auto wait_all = [&](hipStream_t on) {
    if (arrivals)
      for (int c = 0; c < arrivals->count; ++c) (void)hipStreamWaitEvent(on, arrivals->ev[c], 0);
  };
  if (flags & S2K_ECDSA_FORCE_COMPLETE) {
    wait_all(st);
    launch_ecdsa_verify(ctx, st, n, w, pub, dig, r, s, flags, valid);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  const uint32_t T = prep_lanes(n);
  const uint32_t kvf = (flags & S2K_ECDSA_FORCE_WORKLIST) ? KVF_FORCE_WORKLIST : 0u;
  uint64_t* clk = ctx->prof_on ? ctx->clk : nullptr;
  bool grouped = ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH;
  // small batches: a wave per signature beats any table (k_verify_row); a grouping mode somebody asked for by name
  // (S2K_KEYS_AUTO / S2K_KEYS_ALWAYS) is obeyed instead
  const bool row = n <= ctx->row_max && !kvf && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  // ... and up to quad_max four lanes per signature (k_verify_quad): half the latency of the lane kernels for calls that fill
  // neither
  const bool quad = !row && n <= ctx->quad_max && !kvf && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  if (row || quad) grouped = false;
  else HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));      // (these ladders have no worklist: one launch less)
  ctx->kg_note_dst = nullptr;
  if (grouped && ctx->kg_mode == S2K_KEYS_ADAPTIVE && n >= KG_ADAPT_MIN_BATCH) grouped = kg_adaptive_decide(ctx);
  if (grouped) {
    // the grouping arrays and the table buffer, before anything of this call is in flight; a device without room for the
    // tables verifies without them
    rc = s2k_internal_key_reserve(ctx, n, 64);
    if (rc == S2K_ERR_NOMEM) grouped = false;
    else if (rc) return rc;
  }
  ctx->last_wl_count = (row || quad) ? nullptr : w.wl_count;
  prof_mark(ctx, st, 0);
  if (grouped) {
    // Signatures of keys that occur often enough: per-key tables (keyed.hip) and the short ladder; the
    // rest: the general kernel over the list `left`.
    key_groups kg;
    ctx->kt_comb_call = ctx->kt_comb;
    rc = grouped_front(ctx, st, n, pub, 64, w,
                       [&](hipStream_t aux) {
                         if (!arrivals) {
                           launch_scalar_prep(aux, w, 0, n, T, dig, r, s, nullptr, flags);
                           return;
                         }
                         // piece by piece: the planes of the workspace are linear in the signature index, so a piece is
                         // the same kernels on shifted pointers
                         for (int c = 0; c < arrivals->count; ++c) {
                           const size_t lo = arrivals->lo[c], cnt = arrivals->cnt[c];
                           (void)hipStreamWaitEvent(aux, arrivals->ev[c], 0);
                           launch_scalar_prep(aux, w, lo, cnt, prep_lanes(cnt), dig, r, s, nullptr, flags);
                           launch_generator_part(ctx, aux, w, (uint32_t)lo, (uint32_t)(lo + cnt));
                         }
                       },
                       &kg, /*gp_in_prep=*/arrivals != nullptr);
    ctx->kt_comb_call = false;
    if (rc) return rc;
    ctx->kt_last = kg.chunks == KC_TEETH ? S2K_LADDER_COMB : S2K_LADDER_WINDOW;
    prof_mark(ctx, st, 2);
    // the ladder of the tables the grouping built: the comb's, or the window ladder over the 16-bit chunks
    const int keyed_mode = kg.chunks == KC_TEETH ? MODE_ECDSA_COMB : MODE_ECDSA_KEYED;
    launch_ladder(ctx, st, keyed_mode, n, kvf, pub, r, w, valid, nullptr, clk, kg);
    HIP_TRY(ctx, hipGetLastError());
    if (kg.nparts > 1) {   // the other side of the split, once its tables (third stream) are there
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_part1, 0));
      kg.part = 1;
      launch_ladder(ctx, st, keyed_mode, n, kvf, pub, r, w, valid, nullptr, nullptr, kg);
      HIP_TRY(ctx, hipGetLastError());
    }
    prof_mark(ctx, st, 3);
    launch_ladder(ctx, st, MODE_ECDSA_LEFT, n, kvf, pub, r, w, valid, nullptr, nullptr, kg);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 4);
  } else if (quad) {
    // four lanes per signature on the complete formulas (k_verify_quad), behind a preparation with one lane per signature
    wait_all(st);
    launch_scalar_prep(st, w, 0, n, (uint32_t)n, dig, r, s, nullptr, flags);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_verify_quad(ctx, st, n, pub, r, w, valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else if (row) {
    // small batches: a wave per signature on the complete formulas (k_verify_row); nothing is left for the worklist kernel
    wait_all(st);
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_verify_row(ctx, st, n, pub, dig, r, s, flags, valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else {
    wait_all(st);
    launch_scalar_prep(st, w, 0, n, T, dig, r, s, nullptr, flags);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_ladder(ctx, st, MODE_ECDSA, n, kvf, pub, r, w, valid, nullptr, clk, key_groups{});
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
  }
  if (ctx->dbg_gt_swap) {   // test hook: the wide table appears HERE, between the ladder and the kernel that finishes its tagged lanes
    const int bits = ctx->dbg_gt_swap;
    ctx->dbg_gt_swap = 0;
    HIP_TRY(ctx, s2k_internal_gt_debug_publish(ctx->device, bits));
#ifdef S2K_DEBUG_GT_PER_LAUNCH   // (variant build that restores the fault of round 5 - a view per launch - to show the test sees it)
    ctx->gt_call = s2k_internal_gt_load(ctx);
#endif
  }
  launch_verify_fallback(ctx, st, n, w, pub, dig, r, s, flags, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

int s2k_ctx_set_key_grouping(s2k_ctx* ctx, int mode, uint32_t min_group, uint32_t hash_bits, uint32_t max_tables) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (mode != S2K_KEYS_OFF && mode != S2K_KEYS_AUTO && mode != S2K_KEYS_ALWAYS && mode != S2K_KEYS_ADAPTIVE)
    return fail(ctx, S2K_ERR_ARG, "key grouping mode %d", mode);
  if (hash_bits > 30) return fail(ctx, S2K_ERR_ARG, "hash_bits %u > 30", hash_bits);
  ctx->kg_mode = mode;
  ctx->kg_min_group = min_group;
  ctx->kg_hash_bits = hash_bits;
  ctx->kg_max_tables = max_tables ? max_tables : KG_MAX_TABLES_DEFAULT;
  ctx->kg_table_cap = 0;           // (a cap found by an earlier allocation failure is tried afresh)
  return S2K_OK;
}

int s2k_ctx_set_keyed_ladder(s2k_ctx* ctx, int ladder) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (ladder != S2K_LADDER_COMB && ladder != S2K_LADDER_WINDOW) return fail(ctx, S2K_ERR_ARG, "keyed ladder %d", ladder);
  ctx->kt_comb = ladder == S2K_LADDER_COMB;
  return S2K_OK;
}

int s2k_ctx_last_keyed_ladder(s2k_ctx* ctx) { return ctx ? ctx->kt_last : -1; }
int s2k_ctx_last_keyset_ladder(s2k_ctx* ctx) { return ctx ? ctx->ks_last : -1; }

int s2k_ctx_key_grouping_stats(s2k_ctx* ctx, uint32_t* stats) {
  if (!ctx || !stats) return fail(ctx, S2K_ERR_ARG, "null argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (ctx->kg_counters) {
    uint32_t c[KG_COUNTERS];
    HIP_TRY(ctx, hipMemcpy(c, ctx->kg_counters, sizeof c, hipMemcpyDeviceToHost));
    stats[0] = c[KG_NKEYED];
    stats[1] = c[KG_NTAB] < ctx->kg_last_max_tables ? c[KG_NTAB] : ctx->kg_last_max_tables;
    stats[2] = c[KG_NLEFT];
  }
  if (ctx->last_wl_count) HIP_TRY(ctx, hipMemcpy(&stats[3], ctx->last_wl_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return S2K_OK;
}

int s2k_ctx_key_grouping_adaptive(s2k_ctx* ctx, uint32_t* out, int reset) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (out) {
    out[0] = ctx->kga_miss_streak;
    out[1] = ctx->kga_miss_streak >= KG_ADAPT_MISSES ? ctx->kga_skip_left : 0;
    out[2] = ctx->kga_skipped;
    out[3] = ctx->kga_probes;
    out[4] = ctx->kga_observed;
  }
  if (reset) {
    ctx->kga_miss_streak = ctx->kga_skip_left = 0;
    ctx->kga_skipping = false;
    ctx->kga_seen = ctx->kga_seq;                      // notes still on their way are not taken
  }
  return S2K_OK;
}

int s2k_ecdsa_recover_batch_device(s2k_ctx* ctx, size_t n, const void* d_dig, const void* d_r, const void* d_s,
                                   const void* d_recid, uint32_t flags, void* d_pub65, void* d_ok, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_dig || !d_r || !d_s || !d_recid || !d_pub65 || !d_ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  const lane_ws w = lane_ws_of(ctx, n);
  const uint8_t *dig = (const uint8_t*)d_dig, *r = (const uint8_t*)d_r, *s = (const uint8_t*)d_s,
                *rid = (const uint8_t*)d_recid;
  uint8_t *ok = (uint8_t*)d_ok, *pub65 = (uint8_t*)d_pub65;
  if (flags & S2K_ECDSA_FORCE_COMPLETE) {
    launch_recover_fallback(ctx, st, n, w, dig, r, s, rid, ok, pub65);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  // (stage times, s2k_ctx_profile_read_stages: [0] the scalar preparation, [2] the ladder, [3] the shared inversions of the
  // affine results, [4] the worklist)
  prof_mark(ctx, st, 0);
  if (n <= ctx->row_max) {
    // small batches: a wave per item, one launch (k_recover_row: preparation, ladder, inversion and record)
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_recover_row(ctx, st, n, dig, r, s, rid, ok, pub65);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  }
  if (n <= ctx->quad_max) {
    // four lanes per item (k_recover_quad) between a preparation and a finish with one lane per item
    launch_scalar_prep(st, w, 0, n, (uint32_t)n, dig, r, s, rid, 0u);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemsetAsync(d_pub65, 0, n * 65, st));      // items without a key keep the zero record
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_recover_quad(ctx, st, n, r, w, ok);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    launch_affine_finish(st, MODE_RECOVER, n, (uint32_t)n, nullptr, w, ok, pub65);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  }
  HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));
  launch_scalar_prep(st, w, 0, n, prep_lanes(n), dig, r, s, rid, 0u);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemsetAsync(d_pub65, 0, n * 65, st));      // items without a key keep the zero record
  prof_mark(ctx, st, 1);
  prof_mark(ctx, st, 2);
  launch_ladder(ctx, st, MODE_RECOVER, n, 0u, nullptr, r, w, ok, pub65, ctx->prof_on ? ctx->clk : nullptr, key_groups{});
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 3);
  launch_affine_finish(st, MODE_RECOVER, n, (uint32_t)((n + FIN_M - 1) / FIN_M), nullptr, w, ok, pub65);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  launch_recover_worklist(ctx, st, n, w, dig, r, s, rid, ok, pub65);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

int s2k_ecdsa_recover_batch(s2k_ctx* ctx, size_t n, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                            const uint8_t* recid, uint32_t flags, uint8_t* pub65, uint8_t* ok) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!dig || !r || !s || !recid || !pub65 || !ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const stage_part parts[6] = {stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_in(recid, n), stage_out(pub65, n * 65), stage_out(ok, n)};
  return s2k_internal_staged_call(ctx, parts, 6, n * 97, s2k_internal_small_call(ctx, n, flags), [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_recover_batch_device(c, n, d[0], d[1], d[2], d[3], flags, d[4], d[5], st);
  });
}

int s2k_schnorr_verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pk, const void* d_msgs,
                                    const void* d_msg_offsets, size_t msg_len, const void* d_sig, uint32_t flags,
                                    void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_pk || !d_sig || !d_valid || (!d_msgs && (d_msg_offsets || msg_len)))
    return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  const lane_ws w = lane_ws_of(ctx, n);
  const uint8_t* pk = (const uint8_t*)d_pk;
  const uint8_t* sig = (const uint8_t*)d_sig;
  const uint8_t* msgs = (const uint8_t*)d_msgs;
  const uint64_t* offs = (const uint64_t*)d_msg_offsets;
  const uint32_t mlen = (uint32_t)msg_len;
  uint8_t* valid = (uint8_t*)d_valid;
  if (flags & S2K_ECDSA_FORCE_COMPLETE) {
    launch_schnorr_fallback(ctx, st, n, w, pk, sig, msgs, offs, mlen, valid);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  // (stage times, s2k_ctx_profile_read_stages: [0] the front end - challenge hashes, and the grouping and per-key tables when
  // keys repeat -, [2] the ladder over per-key tables or the general one, [3] what the key tables left + the shared inversions,
  // [4] the worklist)
  prof_mark(ctx, st, 0);
  ctx->kg_counters = nullptr;
  ctx->kt_last = -1;
  bool grouped = ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH;
  const bool row = n <= ctx->row_max && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  const bool quad = !row && n <= ctx->quad_max && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  if (row || quad) grouped = false;
  else HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));
  ctx->last_wl_count = (row || quad) ? nullptr : w.wl_count;
  if (grouped) {
    rc = s2k_internal_key_reserve(ctx, n, 32);
    if (rc == S2K_ERR_NOMEM) grouped = false;      // no room for per-key tables: the general ladder for everything
    else if (rc) return rc;
  }
  if (grouped) {
    // signatures that share an x-only key: the grouped flow of the ECDSA path (s2k_ctx_set_key_grouping)
    key_groups kg;
    ctx->kt_comb_call = ctx->kt_comb;
    rc = grouped_front(ctx, st, n, pk, 32, w, [&](hipStream_t aux) { launch_schnorr_prep(aux, n, w, pk, sig, msgs, offs, mlen); }, &kg);
    ctx->kt_comb_call = false;
    if (rc) return rc;
    ctx->kt_last = kg.chunks == KC_TEETH ? S2K_LADDER_COMB : S2K_LADDER_WINDOW;
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    // the ladder of the tables the grouping built: the comb's, or the window ladder over the 16-bit chunks
    const int keyed_mode = kg.chunks == KC_TEETH ? MODE_SCHNORR_COMB : MODE_SCHNORR_KEYED;
    launch_ladder(ctx, st, keyed_mode, n, 0u, pk, sig, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, kg);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    if (kg.nparts > 1) {
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_part1, 0));
      kg.part = 1;
      launch_ladder(ctx, st, keyed_mode, n, 0u, pk, sig, w, valid, nullptr, nullptr, kg);
      HIP_TRY(ctx, hipGetLastError());
    }
    launch_ladder(ctx, st, MODE_SCHNORR_LEFT, n, 0u, pk, sig, w, valid, nullptr, nullptr, kg);
    HIP_TRY(ctx, hipGetLastError());
  } else if (quad) {
    // four lanes per signature (k_schnorr_quad) behind the preparation kernel; nothing left for the finish and worklist kernels
    launch_schnorr_prep(st, n, w, pk, sig, msgs, offs, mlen);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_schnorr_quad(ctx, st, n, pk, sig, w, valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else if (row) {
    // small batches: a wave per signature, nothing left for the finish and worklist kernels (k_schnorr_row): one launch up to
    // 1024 signatures, the preparation kernel in front above
    if (n <= 1024) {
      prof_mark(ctx, st, 1);
      prof_mark(ctx, st, 2);
      launch_schnorr_row(ctx, st, n, pk, sig, msgs, offs, mlen, nullptr, 0, valid);
    } else {
      launch_schnorr_prep(st, n, w, pk, sig, msgs, offs, mlen);
      HIP_TRY(ctx, hipGetLastError());
      prof_mark(ctx, st, 1);
      prof_mark(ctx, st, 2);
      launch_schnorr_row(ctx, st, n, pk, sig, msgs, offs, mlen, w.prep, w.stride, valid);
    }
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else {
    launch_schnorr_prep(st, n, w, pk, sig, msgs, offs, mlen);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_ladder(ctx, st, MODE_SCHNORR, n, 0u, pk, sig, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, key_groups{});
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
  }
  launch_affine_finish(st, MODE_SCHNORR, n, (uint32_t)((n + FIN_M - 1) / FIN_M), sig, w, valid, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  launch_schnorr_worklist(ctx, st, n, w, pk, sig, msgs, offs, mlen, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

// Host-buffer entry point.  The batch is cut into chunks that are whole rounds of k_verify_fast
// on this device (3 waves/SIMD x 4 SIMDs x CUs x 64 lanes; one round first, then two per chunk), and the
// host-to-device copy of chunk j+1 runs on its own stream while chunk j is verified: for pageable
// callers' memory the copy costs about half as much as the verification, so most of it hides.
// Staging buffers and streams live in the context (no hipMalloc per call).
// Everything of a host-buffer verification except the final wait: copies in, kernels, verdicts to h_out (host memory; the
// copy is asynchronous when h_out is page-locked).  All work ends on ctx->s_comp.  one_shot: the batch is not cut into
// chunks (submit / wait: the other slot's batch is what this one's transfer hides behind, and ONE grouped call sees every
// signature of a key).  On an error nothing of the call is left in flight.
static int verify_batch_enqueue_inner(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                      const uint8_t* s, uint32_t flags, uint8_t* h_out, bool one_shot) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  rc = ctx_reserve(ctx, &ctx->io, &ctx->io_bytes, n * 161 + 1024);
  if (rc) return rc;
  uint8_t* d_pub = (uint8_t*)ctx->io;
  uint8_t* d_dig = d_pub + n * 64;
  uint8_t* d_r = d_dig + n * 32;
  uint8_t* d_s = d_r + n * 32;
  uint8_t* d_valid = d_s + n * 32;
  // Pinned host buffers (s2k_host_alloc / s2k_host_register, or the caller's own hipHostMalloc): copies are truly
  // asynchronous, so with the grouping on the whole batch goes through ONE grouped call - the keys are copied first, the
  // grouping and the per-key tables start on them, and the digests and signatures cross PCIe meanwhile (the scalar
  // preparation on the second stream waits for them).  From pageable memory a copy is staged by the runtime and the
  // same order measured slower than two independent halves (9.0 against 8.4-8.6 ms per 2^20), which stay the path there.
  const bool pinned = s2k_internal_host_pinned(pub, n * 64) && s2k_internal_host_pinned(dig, n * 32) && s2k_internal_host_pinned(r, n * 32) &&
                      s2k_internal_host_pinned(s, n * 32);
  // (submit / wait, one_shot: no pieces - the other tickets' kernels are what the transfer hides behind, and the ticket runs
  // one compute stream; measured 5.07 against 5.13 ms per 2^20 with the pieces.  S2K_SUBMIT_ARRIVALS=1: measurement knob)
  static const bool submit_arrivals = [] { const char* v = getenv("S2K_SUBMIT_ARRIVALS"); return v && atoi(v) != 0; }();
  if (pinned && ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH && (!one_shot || submit_arrivals)) {
    rc = ctx_arrival_events(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_pub, pub, n * 64, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_copied[0], ctx->s_copy));
    sig_arrivals arr;
    arr.count = n >= ((size_t)1 << 16) ? 4 : 1;
    const size_t per = ((n + arr.count - 1) / arr.count + 255) & ~(size_t)255;
    for (int c = 0; c < arr.count; ++c) {
      const size_t lo = (size_t)c * per, cnt = lo >= n ? 0 : (n - lo < per ? n - lo : per);
      arr.lo[c] = lo;
      arr.cnt[c] = cnt;
      arr.ev[c] = ctx->ev_arrival[c];
      if (cnt) {
        HIP_TRY(ctx, hipMemcpyAsync(d_r + lo * 32, r + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
        HIP_TRY(ctx, hipMemcpyAsync(d_s + lo * 32, s + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
        HIP_TRY(ctx, hipMemcpyAsync(d_dig + lo * 32, dig + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
      }
      HIP_TRY(ctx, hipEventRecord(arr.ev[c], ctx->s_copy));
    }
    while (arr.count > 1 && arr.cnt[arr.count - 1] == 0) --arr.count;
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_comp, ctx->ev_copied[0], 0));
    rc = verify_batch_device(ctx, n, d_pub, d_dig, d_r, d_s, flags, d_valid, ctx->s_comp, &arr);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_valid, n, hipMemcpyDeviceToHost, ctx->s_comp));
    return S2K_OK;
  }
  const size_t round = (size_t)S2K_FAST_WAVES * 4 * (size_t)ctx->cu_count * 64;
  // chunks are whole rounds of the ladder kernel; the first one is a single round, because its copy is
  // the only one nothing hides (63 -> 31 MB up front at 256 CUs), the others two rounds
  const bool chunked = !one_shot && n > 3 * round;         // small batches: one shot
  // with key grouping on, every chunk groups (and builds tables) on its own, so fewer and larger chunks:
  // two halves, the second copy hidden behind the first half's kernels
  const bool halves = chunked && ctx->kg_mode != S2K_KEYS_OFF;
  int k = 0;
  for (size_t lo = 0, chunk = 0; lo < n; lo += chunk, ++k) {
    chunk = !chunked ? n : halves ? ((n / 2 + 255) & ~(size_t)255) : (lo == 0 ? round : 2 * round);
    if (n - lo < chunk + round) chunk = n - lo;            // no launch of less than a round at the end
    const size_t cnt = chunk;
    // the event of two chunks ago has been waited on by s_comp (in stream order) before it is re-recorded
    HIP_TRY(ctx, hipMemcpyAsync(d_pub + lo * 64, pub + lo * 64, cnt * 64, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipMemcpyAsync(d_dig + lo * 32, dig + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipMemcpyAsync(d_r + lo * 32, r + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipMemcpyAsync(d_s + lo * 32, s + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_copied[k & 1], ctx->s_copy));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_comp, ctx->ev_copied[k & 1], 0));
    rc = s2k_ecdsa_verify_batch_device(ctx, cnt, d_pub + lo * 64, d_dig + lo * 32, d_r + lo * 32, d_s + lo * 32, flags,
                                       d_valid + lo, ctx->s_comp);
    if (rc) return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(h_out, d_valid, n, hipMemcpyDeviceToHost, ctx->s_comp));
  return S2K_OK;
}
static int verify_batch_enqueue(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                const uint8_t* s, uint32_t flags, uint8_t* h_out, bool one_shot) {
  const int rc = verify_batch_enqueue_inner(ctx, n, pub, dig, r, s, flags, h_out, one_shot);
  if (rc) s2k_internal_drain(ctx);
  return rc;
}

int s2k_ecdsa_verify_batch(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                           const uint8_t* s, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!pub || !dig || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  int rc;
  if (s2k_internal_small_call(ctx, n, flags) && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF)) {
    // (ctx_small_block: the wave-per-signature ladder reads the caller's bytes from page-locked memory and writes the verdicts
    // there - no DMA transfers)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ctx_streams(ctx);
    if (rc) return rc;
    const size_t sizes[5] = {n * 64, n * 32, n * 32, n * 32, n};
    uint8_t *h[5], *d[5];
    rc = s2k_internal_small_block(ctx, sizes, 5, h, d);
    if (rc) return rc;
    memcpy(h[0], pub, n * 64);
    memcpy(h[1], dig, n * 32);
    memcpy(h[2], r, n * 32);
    memcpy(h[3], s, n * 32);
    rc = s2k_ecdsa_verify_batch_device(ctx, n, d[0], d[1], d[2], d[3], flags, d[4], ctx->s_comp);
    if (rc) {
      s2k_internal_drain(ctx);
      return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_comp));
    memcpy(valid, h[4], n);
    return S2K_OK;
  }
  rc = verify_batch_enqueue(ctx, n, pub, dig, r, s, flags, valid, /*one_shot=*/false);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->s_comp));
  return S2K_OK;
}

int s2k_ecdsa_verify_batch_submit(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                  const uint8_t* s, uint32_t flags, uint8_t* valid, s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  if (n && (!pub || !dig || !r || !s || !valid)) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  s2k_ctx::pipe_slot* sl = nullptr;
  int rc = s2k_internal_pipe_slot(ctx, n, valid, &sl);
  if (rc) return rc;
  if (n) {
    rc = verify_batch_enqueue(sl->ctx, n, pub, dig, r, s, flags, sl->direct ? valid : sl->h_valid, /*one_shot=*/true);
    if (rc) return fail(ctx, rc, "%s", sl->ctx->err);
  }
  s2k_internal_pipe_issue(ctx, sl, ticket);
  return S2K_OK;
}

// Batches of up to max_n signatures take the wave-per-signature ladder (k_verify_row); 0 switches it off.
int s2k_ctx_set_small_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->row_max = max_n;
  return S2K_OK;
}
// ECDSA batches above that and up to max_n take the four-lanes-per-signature ladder (k_verify_quad); 0 switches it off.
// Key-set calls of up to max_n signatures take the wave-per-signature ladder over the set's tables (k_verify_row_keyset /
// k_schnorr_row_keyset); 0 switches it off.  Comb sets have the threshold below.
int s2k_ctx_set_keyset_small_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->ks_row_max = max_n;
  return S2K_OK;
}
// ... and over a COMB set (k_verify_row_comb / k_schnorr_row_comb), a threshold of its own: 0, the default, is never
int s2k_ctx_set_keyset_comb_small_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->ks_comb_row_max = max_n;
  return S2K_OK;
}
int s2k_ctx_set_mid_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->quad_max = max_n;
  return S2K_OK;
}

int s2k_schnorr_verify_batch(s2k_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* msgs,
                             const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig, uint32_t flags,
                             uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!pk || !sig || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const size_t total = msg_offsets ? (size_t)msg_offsets[n] : n * msg_len, off_bytes = (n + 1) * sizeof(uint64_t);
  if (total && !msgs) return fail(ctx, S2K_ERR_ARG, "null message buffer");
  const stage_part parts[5] = {stage_in(pk, n * 32), stage_in(msgs, total, total ? total : 16), stage_in(msg_offsets, msg_offsets ? off_bytes : 0, off_bytes),
                               stage_in(sig, n * 64), stage_out(valid, n)};
  const bool small = s2k_internal_small_call(ctx, n, flags) && total <= ((size_t)1 << 20);
  return s2k_internal_staged_call(ctx, parts, 5, n * 96 + total, small, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_schnorr_verify_batch_device(c, n, d[0], d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], flags, d[4], st);
  });
}

// Point.DoubleScalarMultBasepointVartime (point_mul_glv.go:307), or scalarMultVartimeGLV (:203) when
// u1 == NULL, over a batch of 65-byte records; host pointers.  impl selects the arithmetic (header).
int s2k_double_scalar_mult_basepoint_batch_ex(s2k_ctx* ctx, uint32_t impl, size_t n, const uint8_t* u1, const uint8_t* u2,
                                              const uint8_t* points, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (impl != S2K_IMPL_COMPLETE && impl != S2K_IMPL_FAST) return fail(ctx, S2K_ERR_ARG, "unknown implementation selector");
  if (n == 0) return S2K_OK;
  if (!u2 || !points || !out) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_u1 = 0, o_u2 = pad(n * 32), o_pts = o_u2 + pad(n * 32), o_out = o_pts + pad(n * 65), o_pub = o_out + pad(n * 65),
               o_ok = o_pub + pad(n * 64), o_status = o_ok + pad(n);
  rc = ctx_reserve(ctx, &ctx->io, &ctx->io_bytes, o_status + 256);
  if (rc) return rc;
  uint8_t* io = (uint8_t*)ctx->io;
  if (u1)
    HIP_TRY(ctx, hipMemcpyAsync(io + o_u1, u1, n * 32, hipMemcpyHostToDevice, st));
  else
    HIP_TRY(ctx, hipMemsetAsync(io + o_u1, 0, n * 32, st));   // plain scalar multiplication: u1 = 0
  HIP_TRY(ctx, hipMemcpyAsync(io + o_u2, u2, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(io + o_pts, points, n * 65, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(io + o_status, 0, 4, st));
  const uint8_t* d_u1 = io + o_u1;
  const lane_ws w = lane_ws_of(ctx, n);
  uint32_t* status = (uint32_t*)(io + o_status);
  if (impl == S2K_IMPL_COMPLETE) {
    launch_point_fallback(ctx, st, /*all=*/true, n, w, d_u1, io + o_u2, io + o_pts, io + o_out, status);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));
    HIP_TRY(ctx, hipMemsetAsync(io + o_out, 0, n * 65, st));   // (the ladder kernel leaves the records of undecided lanes alone)
    launch_hot_prep(st, n, w, d_u1, io + o_u2, io + o_pts, io + o_pub, status);
    HIP_TRY(ctx, hipGetLastError());
    launch_ladder(ctx, st, MODE_POINT, n, 0u, io + o_pub, nullptr, w, io + o_ok, io + o_out, nullptr, key_groups{});
    HIP_TRY(ctx, hipGetLastError());
    launch_affine_finish(st, MODE_RECOVER, n, (uint32_t)((n + FIN_M - 1) / FIN_M), nullptr, w, io + o_ok, io + o_out);
    HIP_TRY(ctx, hipGetLastError());
    launch_point_fallback(ctx, st, /*all=*/false, n, w, d_u1, io + o_u2, io + o_pts, io + o_out, status);
    HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t h_status = 0;
  HIP_TRY(ctx, hipMemcpyAsync(out, io + o_out, n * 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  if (h_status) return fail(ctx, S2K_ERR_ARG, "malformed point record (not an encoding the reference's Point can hold)");
  return S2K_OK;
}

}  // extern "C"
