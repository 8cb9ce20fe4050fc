// worklist.hip — the worklist kernels of the lane-per-signature flows: the lanes a ladder could not decide, once more with
// complete formulas on the 9x29 field (k_verify_fallback, k_verify_fallback_keyset, k_schnorr_worklist, k_recover_worklist), with
// their launchers.  The ladders that fill the worklists: verify_fast.h, comb_ladder.hip; the kernels that take every item
// through the reference-shaped 8x32 path: fallback.hip; the call flows: engine.hip, keyset.hip.
//
// Three ladders are instantiated here and not in a ladder_*.hip unit: k_verify_fast<MODE_SCHNORR>, <MODE_RECOVER> and
// <MODE_SCHNORR_LEFT>, the ones that lift an x-coordinate and so call fe29_sqrt.  fe29_sqrt is not inlined: every unit that
// calls it compiles its own copy, and the compiler hands that copy the occupancy bound of its callers in the unit.  Beside
// ladders alone (all bounded to three waves per SIMD: "amdgpu-waves-per-eu"="3,8" in the unit's IR) its registers are
// allocated differently from the copy every other unit has; beside k_schnorr_worklist and k_recover_worklist, which call it
// without a bound, it is the same code as when the ladders were compiled in engine.hip.
#include "verify_fast.h"

using namespace s2k;

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
    // the fast ladder has established u2 Q == u1 G (verify_fast.h, k_verify_fast: verdict): R = 2 u1 G, from the resident
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
// the ECDSA worklist; the reference-shaped 8x32 versions (fallback.hip) stay for S2K_ECDSA_FORCE_COMPLETE.
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

// One launcher per kernel, as in lane_kernels.hip: it enqueues on the stream it is given and does nothing else.  The worklist
// kernels run on the grid fallback_blocks gives, the kernels that take every item on a thread per item.
__attribute__((visibility("hidden"))) void launch_verify_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pub, const uint8_t* dig,
                                   const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_verify_fallback<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, pub, dig, r, s, flags, out, ctx->gt_call, w.qt, w.stride);
}
__attribute__((visibility("hidden"))) void launch_verify_fallback_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* keys, const uint32_t* kidx,
                                          const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_verify_fallback_keyset<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, keys, kidx, dig, r, s, flags, out, ctx->gt_call, w.qt,
                                                                    w.stride);
}
__attribute__((visibility("hidden"))) void launch_schnorr_worklist(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig,
                                    const uint8_t* msgs, const uint64_t* offs, uint32_t msg_len, uint8_t* out) {
  k_schnorr_worklist<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, pk, sig, msgs, offs, msg_len, out, ctx->gt_call, w.qt,
                                                              w.stride);
}
__attribute__((visibility("hidden"))) void launch_recover_worklist(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* dig, const uint8_t* r,
                                    const uint8_t* s, const uint8_t* recid, uint8_t* ok, uint8_t* pub65) {
  k_recover_worklist<<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, dig, r, s, recid, ok, pub65, ctx->gt_call, w.qt, w.stride);
}

// the three ladders that lift an x-coordinate (see the head of this file)
S2K_LADDER_INSTANCE(MODE_SCHNORR)
S2K_LADDER_INSTANCE(MODE_RECOVER)
S2K_LADDER_INSTANCE(MODE_SCHNORR_LEFT)
