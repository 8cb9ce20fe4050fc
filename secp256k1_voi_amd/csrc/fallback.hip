// fallback.hip — the reference-shaped side of the lane-per-signature flows: the kernels that take every item through the
// complete formulas on the 8x32 field (S2K_ECDSA_FORCE_COMPLETE and its like: k_ecdsa_verify, k_schnorr_fallback,
// k_recover_fallback, k_point_fallback<true>) and the point calls' worklist (k_point_fallback<false>), with their launchers.
// The worklist kernels on the 9x29 field: worklist.hip.  The call flows: engine.hip.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "fe.h"
#include "complete_path.h"
#include "point.h"
#include "sc.h"
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

// One launcher per kernel, as in lane_kernels.hip: it enqueues on the stream it is given and does nothing else.  The worklist
// kernels run on the grid fallback_blocks gives, the kernels that take every item on a thread per item.
__attribute__((visibility("hidden"))) void launch_ecdsa_verify(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pub, const uint8_t* dig,
                                const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_ecdsa_verify<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, pub, dig, r, s, flags, out, ctx->gt_call, w.qt, w.stride);
}
__attribute__((visibility("hidden"))) void launch_schnorr_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig,
                                    const uint8_t* msgs, const uint64_t* offs, uint32_t msg_len, uint8_t* out) {
  k_schnorr_fallback<<<blocks_for(n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, pk, sig, msgs, offs, msg_len, out, ctx->gt_call, w.qt,
                                                    w.stride);
}
__attribute__((visibility("hidden"))) void launch_recover_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* dig, const uint8_t* r,
                                    const uint8_t* s, const uint8_t* recid, uint8_t* ok, uint8_t* pub65) {
  k_recover_fallback<<<blocks_for(n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, dig, r, s, recid, ok, pub65, ctx->gt_call, w.qt, w.stride);
}
__attribute__((visibility("hidden"))) void launch_point_fallback(const s2k_ctx* ctx, hipStream_t st, bool all, size_t n, const lane_ws& w, const uint8_t* u1, const uint8_t* u2,
                                  const uint8_t* pts65, uint8_t* out65, uint32_t* status) {
  if (all)
    k_point_fallback<true><<<blocks_for(n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, u1, u2, pts65, out65, ctx->gt_call, w.qt, w.stride,
                                                          status);
  else
    k_point_fallback<false><<<fallback_blocks(ctx, n), 256, 0, st>>>(w.wl_count, w.wl, (uint32_t)n, u1, u2, pts65, out65, ctx->gt_call, w.qt,
                                                                     w.stride, status);
}
