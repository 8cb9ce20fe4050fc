// rlc.hip — whole-batch verification on gfx950: a batch of BIP-340 or of recoverable ECDSA signatures checked as ONE random
// linear combination, a multiscalar sum that vanishes when every signature verifies (s2k_schnorr_batch_verify_rlc,
// s2k_ecdsa_batch_verify_rlc), and per-signature verdicts at that price by bisecting a rejected batch (the *_bisect calls).
//
// This unit is a customer of the multiscalar core (msm.hip), as msm_seg.hip and pointset.hip are: it asks msm_setup for a
// workspace, writes terms in the format of msm_terms.h and calls msm_core (msm_internal.h).
//   front end      k_schnorr_rlc_prep / k_ecdsa_rlc_prep per signature; the aggregated form groups the keys (keyed.hip) and
//                  adds k_rlc_key_lift / k_ecdsa_key_check and k_rlc_key_terms per distinct key; k_schnorr_rlc_sum the generator's term
//   bisection      rlc_bisect on kept terms: k_rlc_save, k_rlc_gather, k_rlc_mark_valid; the leaves are the ordinary verifiers
//   host           rlc_run_full (coefficient key from the caller's seed and getrandom, mixed with a host SHA-256), staging, the
//                  eight entry points and the two s2k_debug_*_rlc_point hooks
#include <sys/random.h>

#include <vector>

#include "msm_internal.h"
#include "msm_terms.h"
#include "fe29_inv.h"
#include "sc.h"
#include "sha256.h"

namespace {

// ---------------------------------------------------------------------------------------
// BIP-340 batch verification as ONE multi-scalar multiplication (BIP-340 "Batch Verification"):
//   (sum a_i s_i) * G  -  sum a_i * R_i  -  sum (a_i e_i) * P_i  ==  infinity,
// R_i = lift_x(r_i), P_i = lift_x(pk_i), a_0 = 1 and a_i 128-bit values from a keyed PRF
// (SHA-256(seed || i)); the seed is caller-supplied secret randomness.  The reference has
// only the single-signature Verify (schnorr.go:221-253); the contract is
// "batch accepts <=> every single Verify accepts", up to 2^-128.
// Terms, plain form: [0, n) = a_i * (-R_i); [n, 2n) and [2n, 3n) = the two halves of (a_i e_i) * (-P_i);
// 3n, 3n + 1 = the two halves of (sum a_i s_i) * G.
// Aggregated form (the whole-batch verdict; keys repeat in real batches): the signatures are grouped by key
// (keyed.hip) and each distinct key P contributes ONE term pair (sum over its signatures of a_i e_i) * (-P):
// [0, n) as before, n + 2t, n + 2t + 1 for group t, then the generator's pair.  One square root per distinct
// key instead of one per signature, n + 2 K + 2 terms instead of 3 n + 2.  The sum is the same group
// element, so the error point of a rejected batch can seed the bisection, which works on the plain form.
// ---------------------------------------------------------------------------------------
S2K_DEV bool lift_x_words(uint32_t yw[8], const uint32_t xw[8]) {
  if (!fe_is_canonical_raw(xw)) return false;
  fe29 x = fe29_from_words(xw);
  fe29 rhs = fe29_mul(fe29_sqr(x), x);
  rhs.n[0] += 7;
  fe29 y;
  if (!fe29_sqrt(y, rhs)) return false;
  y = fe29_normalize(y);
  y = fe29_normalize(fe29_select((y.n[0] & 1u) != 0, y, fe29_negate(y, 1)));   // even root
  fe29_to_words(yw, y);
  return true;
}
// the root whose parity is `odd` (0 / 1): the even root, or p minus it (p is odd and y != 0 on this curve)
S2K_DEV bool lift_x_parity_words(uint32_t yw[8], const uint32_t xw[8], uint32_t odd) {
  uint32_t even[8], other[8];
  if (!lift_x_words(even, xw)) return false;
  u256_sub(other, FE_P, even);
#pragma unroll
  for (int w = 0; w < 8; ++w) yw[w] = odd ? other[w] : even[w];
  return true;
}
// a_i = low 128 bits of SHA-256(key || i), a_0 = 1: the coefficients of the whole-batch checks
S2K_DEV sc rlc_coefficient(const uint32_t key_be[8], size_t i) {
  sc a = sc_zero();
  if (i == 0) {
    a.v[0] = 1;
    return a;
  }
  uint32_t st[8], w[16];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    st[j] = SHA256_IV[j];
    w[j] = key_be[j];
  }
  w[8] = (uint32_t)(i >> 32);
  w[9] = (uint32_t)i;
  w[10] = 0x80000000u;
  w[11] = w[12] = w[13] = w[14] = 0;
  w[15] = 40 * 8;
  sha256_compress(st, w);
  a.v[0] = st[7]; a.v[1] = st[6]; a.v[2] = st[5]; a.v[3] = st[4];
  return a;
}

struct rlc_key {   // PRF key of the coefficients, passed by value as a kernel argument
  uint32_t w[8];
};
// AGG: the key terms are left to k_rlc_key_terms (one term pair per DISTINCT key, its coefficient the sum of
// a_i e_i over the key's signatures): this kernel stores a_i e_i in ae_out instead, and neither lifts nor
// judges the key.  N: plane stride of the term arrays (3n + 2 plain, n + 2 (groups) + 2 aggregated).
template <bool AGG>
__global__ void __launch_bounds__(256)
k_schnorr_rlc_prep(uint32_t n, size_t N, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig,
                   const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
                   rlc_key seed_be, uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw,
                   uint8_t* __restrict__ flag, uint32_t* __restrict__ as_out, uint32_t* __restrict__ ae_out,
                   uint32_t* __restrict__ status) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t r_le[8], pk_le[8];
  sc s;
  load_be32(r_le, sig + i * 64);
  load_be32(s.v, sig + i * 64 + 32);
  load_be32(pk_le, pk + i * 32);
  bool ok = sc_is_canonical_raw(s.v);
  uint32_t ry[8], py[8];
  ok = lift_x_words(ry, r_le) && ok;      // r < p and on the curve (BIP-340 batch: fail if lift fails)
  if constexpr (!AGG) ok = lift_x_words(py, pk_le) && ok;
  if (!ok) atomicOr(status, 2u);
  // e_i
  uint32_t r_be[8], pk_be[8], dg[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    r_be[w] = r_le[7 - w];
    pk_be[w] = pk_le[7 - w];
  }
  const uint8_t* m = offs ? msgs + offs[i] : msgs + i * (size_t)msg_len;
  uint32_t len = offs ? (uint32_t)(offs[i + 1] - offs[i]) : msg_len;
  bip340_challenge(dg, r_be, pk_be, m, len);
  uint32_t e_raw[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) e_raw[w] = dg[7 - w];
  sc e = sc_reduce_once(e_raw);
  const sc a = rlc_coefficient(seed_be.w, i);
  sc a_m = sc_to_mont(a);
  sc ae = sc_montmul(e, a_m), as = sc_montmul(s, a_m);
  // -a_i * R_i and -(a_i e_i) * P_i are entered as a_i * (-R_i) and (a_i e_i) * (-P_i): negating the
  // point is free, whereas n - a_i (a_i < 2^128) would put every R term into the same 0xFFFF
  // buckets of the upper windows and serialise them on single lanes.
  if (ok) msm_store_term(scw, ptw, N, i, a, r_le, ry, true);                          // a_i < 2^128 already
  if constexpr (AGG) {
    // (a 32-byte record per signature, not planes: k_rlc_key_terms gathers them by key, from all over the array - eight
    // 4-byte reads per member, each a memory transaction of its own, were most of that kernel's 0.070 ms; now 0.035)
    uint4* rec = reinterpret_cast<uint4*>(ae_out + (size_t)i * 8);
    rec[0] = make_uint4(ae.v[0], ae.v[1], ae.v[2], ae.v[3]);
    rec[1] = make_uint4(ae.v[4], ae.v[5], ae.v[6], ae.v[7]);
  } else {
    uint32_t npy[8];
    u256_sub(npy, FE_P, py);
    if (ok) msm_store_split(scw, ptw, N, (size_t)n + i, 2 * (size_t)n + i, ae, pk_le, npy);
    flag[(size_t)n + i] = ok ? 1 : 0;
    flag[2 * (size_t)n + i] = ok ? 1 : 0;
  }
  // a signature whose r or key does not lift is invalid on its own; it takes no part in the combination
#pragma unroll
  for (int w = 0; w < 8; ++w) as_out[(size_t)w * n + i] = ok ? as.v[w] : 0u;
  flag[i] = ok ? 1 : 0;
}

// Recoverable ECDSA signatures as the same kind of sum (header: s2k_ecdsa_batch_verify_rlc):
//   sum a_i * R_i  -  (sum a_i u1_i) * G  -  sum (a_i u2_i) * Q_i  ==  infinity,   u1 = e / s, u2 = r / s, R_i = RecoverPoint(r_i, v_i),
// in the layouts of the BIP-340 forms above.  Terms [0, n) = a_i * R_i (a 128-bit coefficient, never negated); the key terms
// are (a_i u2_i) * (-Q_i), negated on the point as there - per signature at [n, 2n) and [2n, 3n) in the plain form, per
// distinct key behind n in the aggregated one (ae_out gets a_i u2_i; k_ecdsa_key_check judges the keys, k_rlc_key_terms sums);
// as_out gets a_i u1_i, whose sum k_schnorr_rlc_sum enters negated with G.  An item that fails one of its own checks
// (ranges of r and s, low s under the flag, v, x = r + n below p, x on the curve; plain form: its key) leaves the combination.
// One lane per signature with an inversion of its own (sc_modinv: safegcd): no lane shares a product with another, so an s
// that has no inverse cannot spoil a neighbour's (the simpler of the two ways; k_scalar_prep's shared inversion would save most of it).
template <bool AGG>
__global__ void __launch_bounds__(256)
k_ecdsa_rlc_prep(uint32_t n, size_t N, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ dig,
                 const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig, const uint8_t* __restrict__ recid,
                 uint32_t flags, rlc_key seed_be, uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw,
                 uint8_t* __restrict__ flag, uint32_t* __restrict__ as_out, uint32_t* __restrict__ ae_out,
                 uint32_t* __restrict__ status) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  sc r, s;
  uint32_t e_raw[8];
  load_be32(r.v, rsig + i * 32);
  load_be32(s.v, ssig + i * 32);
  load_be32(e_raw, dig + i * 32);
  const uint32_t v = recid[i];
  const bool s_ok = sc_is_canonical_raw(s.v) && !sc_is_zero(s);
  bool ok = sc_is_canonical_raw(r.v) && !sc_is_zero(r) && s_ok && v <= 3u;
  if (flags & S2K_ECDSA_REJECT_MALLEABLE) ok = ok && !sc_is_gt_half_n(s);
  // RecoverPoint (point_s11n.go:245-282): bit 1 of v means x = r + n, which must stay below p; bit 0 is the parity of y
  uint32_t xw[8], ry[8];
  {
    uint32_t rn[8];
    const uint32_t carry = u256_add(rn, r.v, SC_N);
    const bool high = (v & 2u) != 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) xw[w] = high ? rn[w] : r.v[w];
    ok = ok && !(high && carry != 0);
  }
  ok = lift_x_parity_words(ry, xw, v & 1u) && ok;          // (refuses x >= p)
  uint32_t qx[8], qy[8];
  if constexpr (!AGG) {
    load_be32(qx, pub + i * 64);
    load_be32(qy, pub + i * 64 + 32);
    ok = xy_on_curve_words(qx, qy) && ok;
  }
  if (!ok) atomicOr(status, 2u);
  sc s_inv = s;
  if (!s_ok) {            // (rejected above; the inversion wants a canonical value)
    s_inv = sc_zero();
    s_inv.v[0] = 1;
  }
  const sc s_inv_m = sc_to_mont(sc_modinv(s_inv));
  const sc e = sc_reduce_once(e_raw);
  const sc a = rlc_coefficient(seed_be.w, i);
  const sc a_m = sc_to_mont(a);
  const sc au1 = sc_montmul(sc_montmul(e, s_inv_m), a_m), au2 = sc_montmul(sc_montmul(r, s_inv_m), a_m);
  if (ok) msm_store_term(scw, ptw, N, i, a, xw, ry, false);                           // a_i < 2^128 already
  if constexpr (AGG) {
    uint4* rec = reinterpret_cast<uint4*>(ae_out + (size_t)i * 8);
    rec[0] = make_uint4(au2.v[0], au2.v[1], au2.v[2], au2.v[3]);
    rec[1] = make_uint4(au2.v[4], au2.v[5], au2.v[6], au2.v[7]);
  } else {
    uint32_t nqy[8];
    u256_sub(nqy, FE_P, qy);
    if (ok) msm_store_split(scw, ptw, N, (size_t)n + i, 2 * (size_t)n + i, au2, qx, nqy);
    flag[(size_t)n + i] = ok ? 1 : 0;
    flag[2 * (size_t)n + i] = ok ? 1 : 0;
  }
#pragma unroll
  for (int w = 0; w < 8; ++w) as_out[(size_t)w * n + i] = ok ? au1.v[w] : 0u;
  flag[i] = ok ? 1 : 0;
}
// The aggregated form's keys are X || Y: no square root per key, only NewPublicKey's validation, once per group
// (ky[w][t] = Y, kok[t] = 1 if the key is a point of the curve: what k_rlc_key_lift leaves for x-only keys).
__global__ void __launch_bounds__(64)
k_ecdsa_key_check(uint32_t ngroups, uint32_t nleft, size_t kstride, const uint32_t* __restrict__ vslot, const uint32_t* __restrict__ rep,
                  const uint32_t* __restrict__ left, const uint8_t* __restrict__ pub, uint32_t* __restrict__ ky, uint8_t* __restrict__ kok) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= ngroups + nleft) return;
  const uint32_t key_sig = t < ngroups ? rep[vslot[t]] : left[t - ngroups];
  uint32_t qx[8], qy[8];
  load_be32(qx, pub + (size_t)key_sig * 64);
  load_be32(qy, pub + (size_t)key_sig * 64 + 32);
  const bool key_ok = xy_on_curve_words(qx, qy);
#pragma unroll
  for (int w = 0; w < 8; ++w) ky[(size_t)w * kstride + t] = key_ok ? qy[w] : 0u;
  kok[t] = key_ok ? 1 : 0;
}
// The leaf of the ECDSA bisection, behind s2k_ecdsa_recover_batch_device: valid[i] = RecoverPublicKey succeeded and returned
// exactly the supplied key (k.Equal(q) compares the serialised points, secec.go:121-129; a recovered key is a canonical point
// of the curve, so a supplied key that NewPublicKey refuses equals none), and s <= n/2 under the flag.
__global__ void __launch_bounds__(256)
k_ecdsa_rlc_leaf(uint32_t n, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ ssig, uint32_t flags,
                 const uint8_t* __restrict__ rec65, const uint8_t* __restrict__ ok, uint8_t* __restrict__ valid) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t* a = pub + i * 64;
  const uint8_t* b = rec65 + i * 65;
  uint32_t diff = b[0] ^ 0x04u;
  for (int j = 0; j < 64; ++j) diff |= (uint32_t)(a[j] ^ b[1 + j]);
  bool good = ok[i] == 1 && diff == 0;
  if (flags & S2K_ECDSA_REJECT_MALLEABLE) {
    sc s;
    load_be32(s.v, ssig + i * 32);
    good = good && !sc_is_gt_half_n(s);
  }
  valid[i] = good ? 1 : 0;
}

// Aggregated key terms, in two kernels.  Lane t < ngroups: virtual group t (the signatures perm[first .. first + count)
// of one key); lane ngroups + q: the signature left[q] on its own.
// k_rlc_key_lift lifts the group's key ONCE (a square root: the expensive part; it needs the grouping only, so it runs on
// the second stream beside k_schnorr_rlc_prep): ky[w][t] = the even y, kok[t] = 1 if the key lifts.
__global__ void __launch_bounds__(64)
k_rlc_key_lift(uint32_t ngroups, uint32_t nleft, size_t kstride, const uint32_t* __restrict__ vslot, const uint32_t* __restrict__ rep,
               const uint32_t* __restrict__ left, const uint8_t* __restrict__ pk, uint32_t* __restrict__ ky, uint8_t* __restrict__ kok) {
  const uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= ngroups + nleft) return;
  const uint32_t key_sig = t < ngroups ? rep[vslot[t]] : left[t - ngroups];
  uint32_t pk_le[8], py[8];
  load_be32(pk_le, pk + (size_t)key_sig * 32);
  const bool key_ok = lift_x_words(py, pk_le);
#pragma unroll
  for (int w = 0; w < 8; ++w) ky[(size_t)w * kstride + t] = key_ok ? py[w] : 0u;
  kok[t] = key_ok ? 1 : 0;
}
// k_rlc_key_terms: the group's coefficient is the sum of a_i e_i over its members that are still in the combination
// (flag).  A key that does not lift takes its signatures out of the combination (flag, a_i s_i) and fails the batch
// (status).  Terms n + 2t, n + 2t + 1 (N: plane stride of the term arrays).  KEYBYTES: 32 (x-only, BIP-340) or 64 (X || Y, ECDSA);
// either way the term's point is the key's (x, -y), y from ky.
template <int KEYBYTES>
__global__ void __launch_bounds__(64)
k_rlc_key_terms(uint32_t n, size_t N, uint32_t ngroups, uint32_t nleft, const uint32_t* __restrict__ vslot,
                const uint32_t* __restrict__ rep, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ base,
                const uint32_t* __restrict__ tix, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ left,
                const uint8_t* __restrict__ pk, size_t kstride, const uint32_t* __restrict__ ky, const uint8_t* __restrict__ kok,
                const uint32_t* __restrict__ ae, uint32_t* __restrict__ as_io,
                uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw, uint8_t* __restrict__ flag,
                uint32_t* __restrict__ status) {
  uint32_t t = blockIdx.x * 64 + threadIdx.x;
  if (t >= ngroups + nleft) return;
  uint32_t first = 0, count = 1, key_sig;
  const uint32_t* members;
  if (t < ngroups) {
    const uint32_t s = vslot[t], v = t - tix[s];
    first = base[s] + v * KG_VGROUP;
    const uint32_t rest = cnt[s] - v * KG_VGROUP;
    count = rest < KG_VGROUP ? rest : KG_VGROUP;
    key_sig = rep[s];
    members = perm;
  } else {
    first = t - ngroups;
    key_sig = left[first];
    members = left;
  }
  const bool key_ok = kok[t] != 0;
  sc sum = sc_zero();
  bool any = false;
#pragma unroll 1
  for (uint32_t j = 0; j < count; ++j) {
    const size_t i = members[first + j];
    if (!flag[i]) continue;
    if (!key_ok) {   // out of the combination
      flag[i] = 0;
#pragma unroll
      for (int w = 0; w < 8; ++w) as_io[(size_t)w * n + i] = 0u;
      continue;
    }
    const uint4* rec = reinterpret_cast<const uint4*>(ae + i * 8);
    const uint4 lo4 = rec[0], hi4 = rec[1];
    sc v;
    v.v[0] = lo4.x; v.v[1] = lo4.y; v.v[2] = lo4.z; v.v[3] = lo4.w;
    v.v[4] = hi4.x; v.v[5] = hi4.y; v.v[6] = hi4.z; v.v[7] = hi4.w;
    sum = sc_add(sum, v);
    any = true;
  }
  if (!key_ok) atomicOr(status, 2u);
  const size_t t1 = (size_t)n + 2 * (size_t)t, t2 = t1 + 1;
  if (key_ok && any) {
    uint32_t pk_le[8], py[8], npy[8];
    load_be32(pk_le, pk + (size_t)key_sig * KEYBYTES);
#pragma unroll
    for (int w = 0; w < 8; ++w) py[w] = ky[(size_t)w * kstride + t];
    u256_sub(npy, FE_P, py);
    msm_store_split(scw, ptw, N, t1, t2, sum, pk_le, npy);
    flag[t1] = 1;
    flag[t2] = 1;
  }
}

// sum of n scalars mod n in two launches: RLC_SUM_BLOCKS workgroups leave one partial sum each in
// `part` (8 words each), then one workgroup folds those and writes the result as terms 3n, 3n + 1
// with the point G (as == nullptr selects the second stage) - with -G when `negate` (the ECDSA form subtracts the generator's
// term; the full-width coefficient is negated, it is split anyway); N terms in arrays of plane stride tstride
constexpr uint32_t RLC_SUM_BLOCKS = 256;
// (`as` has plane stride `stride`; a sub-range of a saved batch passes as + lo with the batch's stride)
__global__ void __launch_bounds__(256)
k_schnorr_rlc_sum(uint32_t n, size_t stride, const uint32_t* __restrict__ as, uint32_t* __restrict__ part,
                  uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw, uint8_t* __restrict__ flag, size_t N, size_t tstride,
                  uint32_t negate) {
  __shared__ uint32_t sh[256][8];
  sc acc = sc_zero();
  if (as) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)RLC_SUM_BLOCKS * 256) {
      sc v;
#pragma unroll
      for (int w = 0; w < 8; ++w) v.v[w] = as[(size_t)w * stride + i];
      acc = sc_add(acc, v);
    }
  } else if (threadIdx.x < RLC_SUM_BLOCKS) {
#pragma unroll
    for (int w = 0; w < 8; ++w) acc.v[w] = part[threadIdx.x * 8 + w];
  }
#pragma unroll
  for (int w = 0; w < 8; ++w) sh[threadIdx.x][w] = acc.v[w];
  __syncthreads();
  for (uint32_t half = 128; half >= 1; half >>= 1) {
    if (threadIdx.x < half) {
      sc a, b;
#pragma unroll
      for (int w = 0; w < 8; ++w) {
        a.v[w] = sh[threadIdx.x][w];
        b.v[w] = sh[threadIdx.x + half][w];
      }
      a = sc_add(a, b);
#pragma unroll
      for (int w = 0; w < 8; ++w) sh[threadIdx.x][w] = a.v[w];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  if (as) {
#pragma unroll
    for (int w = 0; w < 8; ++w) part[blockIdx.x * 8 + w] = sh[0][w];
  } else {
    sc tot;                                   // the generator's terms are the last two of the N
#pragma unroll
    for (int w = 0; w < 8; ++w) tot.v[w] = sh[0][w];
    if (negate) tot = sc_neg(tot);
    msm_store_split(scw, ptw, tstride, N - 2, N - 1, tot, FE_GX, FE_GY);
    flag[N - 2] = 1;
    flag[N - 1] = 1;
  }
}

// ---------------------------------------------------------------------------------------
// Locating the failing signatures of a rejected batch.  The terms of the whole
// batch (coefficients, challenges times coefficients, lifted points: the expensive part of the
// preparation) are kept; a sub-range [lo, lo + m) of the signatures is re-checked by gathering its
// 3m terms into a fresh term array, summing its a_i s_i for the generator term and running the
// multiscalar core on 3m + 2 terms.  The result is the range's error point E = sum of the
// coefficients times the individual errors; E_right = E_parent - E_left, so every level costs one
// multiscalar multiplication of half its parent's size.
// Saved layout: s_scw [4][3n] (magnitudes), s_ptw [3n][16], s_flag [n], s_as [8][n].
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_rlc_gather(uint32_t lo, uint32_t m, uint32_t n, const uint32_t* __restrict__ s_scw, const uint32_t* __restrict__ s_ptw,
             const uint8_t* __restrict__ s_flag, uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw,
             uint8_t* __restrict__ flag) {
  size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;     // destination term among the 3m
  if (j >= 3 * (size_t)m) return;
  const size_t part = j / m, i = j - part * m;            // 0: R terms, 1 and 2: the halves of the P terms
  const size_t src = part * n + lo + i, N = 3 * (size_t)m + 2, NS = 3 * (size_t)n;
  msm_copy_term<true>(scw, ptw, N, j, s_scw, s_ptw, NS, src);
  flag[j] = s_flag[lo + i];
}
// terms of the whole batch -> saved arrays (3n + 2 -> 3n: the generator terms are rebuilt per range)
__global__ void __launch_bounds__(256)
k_rlc_save(uint32_t n, const uint32_t* __restrict__ scw, const uint32_t* __restrict__ ptw, const uint8_t* __restrict__ flag,
           uint32_t* __restrict__ s_scw, uint32_t* __restrict__ s_ptw, uint8_t* __restrict__ s_flag) {
  size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= 3 * (size_t)n) return;
  const size_t N = 3 * (size_t)n + 2, NS = 3 * (size_t)n;
  msm_copy_term<false>(s_scw, s_ptw, NS, j, scw, ptw, N, j);
  if (j < n) s_flag[j] = flag[j];
}
// valid[lo + i] = ok-to-lift flag of signature lo + i (a range the combination has cleared)
__global__ void __launch_bounds__(256)
k_rlc_mark_valid(uint32_t lo, uint32_t m, const uint8_t* __restrict__ s_flag, uint8_t* __restrict__ valid) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) valid[lo + i] = s_flag[lo + i];
}

}  // namespace

extern "C" {

// SHA-256 on the host (FIPS 180-4), for mixing the caller's seed with operating-system randomness
static void host_sha256(uint8_t out[32], const uint8_t* msg, size_t len) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t st[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  uint8_t buf[128];
  size_t full = len / 64, rem = len % 64;
  auto block = [&](const uint8_t* b) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    for (int i = 16; i < 64; ++i) {
      uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = st[0], bb = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], hh = st[7];
    for (int i = 0; i < 64; ++i) {
      uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g), t1 = hh + S1 + ch + K[i] + w[i];
      uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & bb) ^ (a & c) ^ (bb & c), t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = bb; bb = a; a = t1 + t2;
    }
    st[0] += a; st[1] += bb; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += hh;
  };
  for (size_t i = 0; i < full; ++i) block(msg + 64 * i);
  memset(buf, 0, sizeof buf);
  memcpy(buf, msg + 64 * full, rem);
  buf[rem] = 0x80;
  size_t padded = rem + 9 <= 64 ? 64 : 128;
  uint64_t bits = (uint64_t)len * 8;
  for (int i = 0; i < 8; ++i) buf[padded - 1 - i] = (uint8_t)(bits >> (8 * i));
  block(buf);
  if (padded == 128) block(buf + 64);
  for (int i = 0; i < 8; ++i) {
    out[4 * i] = (uint8_t)(st[i] >> 24); out[4 * i + 1] = (uint8_t)(st[i] >> 16); out[4 * i + 2] = (uint8_t)(st[i] >> 8); out[4 * i + 3] = (uint8_t)st[i];
  }
}

// stage (pk, msgs, offsets, sig [, valid]) of a BIP-340 batch in the context's buffers on its compute stream
static int stage_schnorr(s2k_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* msgs, const uint64_t* msg_offsets, size_t msg_len,
                         const uint8_t* sig, uint8_t* d[5], hipStream_t* st_out) {
  size_t total = msg_offsets ? (size_t)msg_offsets[n] : n * msg_len;
  if (total && !msgs) return fail(ctx, S2K_ERR_ARG, "null message buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  const size_t sizes[5] = {n * 32, total ? total : 16, (n + 1) * sizeof(uint64_t), n * 64, n};
  rc = ctx_stage(ctx, sizes, 5, d);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  HIP_TRY(ctx, hipMemcpyAsync(d[0], pk, n * 32, hipMemcpyHostToDevice, st));
  if (total) HIP_TRY(ctx, hipMemcpyAsync(d[1], msgs, total, hipMemcpyHostToDevice, st));
  if (msg_offsets) HIP_TRY(ctx, hipMemcpyAsync(d[2], msg_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(d[3], sig, n * 64, hipMemcpyHostToDevice, st));
  *st_out = st;
  return S2K_OK;
}

// whole-batch combination: preparation, generator term, multiscalar core; leaves the 129 bytes
// [status word .. 64: error point record] in h.  The caller's seed is mixed with 32 bytes from the
// operating system's CSPRNG, so a reused or predictable seed does not weaken the check (the
// coefficients have to be unpredictable to whoever chose the signatures).
enum rlc_mode {
  RLC_AGGREGATED,        // one term pair per distinct key; combination evaluated
  RLC_PLAIN_TERMS_ONLY   // one term pair per signature (the layout the bisection gathers from); terms only
};
// The two signature schemes that are checked this way share everything behind their front end: the term arrays and
// their two layouts, the grouping of the keys, the key terms, the generator's term, the multiscalar core, the bisection.
enum rlc_scheme { RLC_BIP340, RLC_ECDSA };
struct rlc_batch {        // the device pointers of one batch
  rlc_scheme scheme;
  const uint8_t* key;     // BIP-340: x-only keys, 32 bytes each; ECDSA: X || Y, 64 bytes each
  // BIP-340
  const uint8_t* msgs;
  const uint64_t* msg_offsets;
  size_t msg_len;
  const uint8_t* sig;
  // ECDSA, recoverable signatures
  const uint8_t *dig, *r, *s, *recid;
  uint32_t flags;         // S2K_ECDSA_REJECT_MALLEABLE
};
static rlc_batch rlc_batch_bip340(const void* d_pk, const void* d_msgs, const void* d_msg_offsets, size_t msg_len, const void* d_sig) {
  rlc_batch b{};
  b.scheme = RLC_BIP340;
  b.key = (const uint8_t*)d_pk;
  b.msgs = (const uint8_t*)d_msgs;
  b.msg_offsets = (const uint64_t*)d_msg_offsets;
  b.msg_len = msg_len;
  b.sig = (const uint8_t*)d_sig;
  return b;
}
static rlc_batch rlc_batch_ecdsa(const void* d_pub, const void* d_dig, const void* d_r, const void* d_s, const void* d_recid, uint32_t flags) {
  rlc_batch b{};
  b.scheme = RLC_ECDSA;
  b.key = (const uint8_t*)d_pub;
  b.dig = (const uint8_t*)d_dig;
  b.r = (const uint8_t*)d_r;
  b.s = (const uint8_t*)d_s;
  b.recid = (const uint8_t*)d_recid;
  b.flags = flags;
  return b;
}
// `seed_be`: the coefficient key; derived here from seed32 and OS randomness when `fresh`, otherwise taken
// as it is (a second pass over the same batch must use the coefficients of the first).
static int rlc_run_full(s2k_ctx* ctx, hipStream_t st, size_t n, const rlc_batch& in, const uint8_t* seed32, msm_ws& m,
                        uint32_t** as_out, uint8_t h[192], rlc_mode mode, rlc_key& seed_be, bool fresh) {
  const bool ecdsa = in.scheme == RLC_ECDSA;
  if (fresh) {
    uint8_t mix[64], key[32];
    memcpy(mix, seed32, 32);
    if (getrandom(mix + 32, 32, 0) != 32) return fail(ctx, S2K_ERR_HIP, "getrandom failed: no randomness for the batch coefficients");
    host_sha256(key, mix, 64);
    for (int j = 0; j < 8; ++j)
      seed_be.w[j] = ((uint32_t)key[4 * j] << 24) | ((uint32_t)key[4 * j + 1] << 16) | ((uint32_t)key[4 * j + 2] << 8) | key[4 * j + 3];
  }
  // The workspace is carved for the plain form's 3n + 2 terms in both modes (the aggregated form has fewer, but how many
  // is known only once the keys are grouped, and the preparation must not wait for that): `cap` is the plane stride.
  const size_t cap = 3 * n + 2;
  size_t N = cap;
  // aux: 256 bytes | partial sums of the generator's coefficient | a_i s_i planes | a_i e_i records, lifted keys (aggregated)
  // (ECDSA: a_i u1_i planes, a_i u2_i records, the keys' Y)
  const size_t as_bytes = n * 8 * 4, kstride = (n + 63) & ~(size_t)63;
  int rc = msm_setup(ctx, cap, 256 + RLC_SUM_BLOCKS * 32 + as_bytes + (mode == RLC_AGGREGATED ? as_bytes + kstride * 36 : 0), m);
  if (rc) return rc;
  uint32_t* sum_part = (uint32_t*)(m.aux + 256);
  uint32_t* as = (uint32_t*)(m.aux + 256 + RLC_SUM_BLOCKS * 32);
  uint32_t* ae = as + n * 8;
  uint32_t* ky = ae + n * 8;
  uint8_t* kok = (uint8_t*)(ky + kstride * 8);
  msm_prof_mark(ctx, st, 0);
  HIP_TRY(ctx, msm_clear(ctx, st, m));
  if (mode == RLC_AGGREGATED) {
    // Two streams.  Caller's: the per-signature preparation (challenge hash, square root of r, coefficients: 1.2 ms of
    // multiplier time for 2^20 signatures).  Second: the grouping of the keys (hash table, latency bound; it ends with
    // the one host read of the call, the group count) and one square root per DISTINCT key.  They meet at the key terms.
    rc = ctx_aux_streams(ctx);
    if (rc) return rc;
    rc = s2k_internal_key_reserve32(ctx, n);   // the grouping arrays are grown before the fork (growing synchronises the device)
    if (rc) return rc;
    HIP_TRY(ctx, hipMemsetAsync(m.flag, 0, cap, st));     // the key terms set their own flags
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux, ctx->ev_fork, 0));
    if (ecdsa)
      k_ecdsa_rlc_prep<true><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, cap, in.key, in.dig, in.r, in.s, in.recid, in.flags, seed_be,
                                                            m.scw, m.ptw, m.flag, as, ae, m.status);
    else
      k_schnorr_rlc_prep<true><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, cap, in.key, in.sig, in.msgs, in.msg_offsets,
                                                              (uint32_t)in.msg_len, seed_be, m.scw, m.ptw, m.flag, as, ae, m.status);
    key_groups32 kg;
    rc = hipGetLastError() == hipSuccess ? S2K_OK : fail(ctx, S2K_ERR_HIP, "whole-batch preparation: launch failed");
    if (rc == S2K_OK) rc = s2k_internal_key_group_all(ctx, n, in.key, ecdsa ? 64 : 32, ctx->s_aux, &kg);   // (synchronises the second stream)
    uint32_t lanes = 0;
    if (rc == S2K_OK) {
      lanes = kg.ngroups + kg.nleft;
      N = n + 2 * (size_t)lanes + 2;
      if (ecdsa)
        k_ecdsa_key_check<<<(lanes + 63) / 64, 64, 0, ctx->s_aux>>>(kg.ngroups, kg.nleft, kstride, kg.vslot, kg.rep, kg.left, in.key, ky, kok);
      else
        k_rlc_key_lift<<<(lanes + 63) / 64, 64, 0, ctx->s_aux>>>(kg.ngroups, kg.nleft, kstride, kg.vslot, kg.rep, kg.left, in.key, ky, kok);
      if (hipGetLastError() != hipSuccess) rc = fail(ctx, S2K_ERR_HIP, "whole-batch key check: launch failed");
    }
    ctx_aux_join(ctx, st);            // error or not: nothing stays in flight on the second stream alone
    if (rc) {
      (void)ctx_leave(ctx, st);
      return rc;
    }
    if (ecdsa)
      k_rlc_key_terms<64><<<(lanes + 63) / 64, 64, 0, st>>>((uint32_t)n, cap, kg.ngroups, kg.nleft, kg.vslot, kg.rep, kg.cnt, kg.base, kg.tix,
                                                            kg.perm, kg.left, in.key, kstride, ky, kok, ae, as, m.scw, m.ptw, m.flag, m.status);
    else
      k_rlc_key_terms<32><<<(lanes + 63) / 64, 64, 0, st>>>((uint32_t)n, cap, kg.ngroups, kg.nleft, kg.vslot, kg.rep, kg.cnt, kg.base, kg.tix,
                                                            kg.perm, kg.left, in.key, kstride, ky, kok, ae, as, m.scw, m.ptw, m.flag, m.status);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    if (ecdsa)
      k_ecdsa_rlc_prep<false><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, cap, in.key, in.dig, in.r, in.s, in.recid, in.flags, seed_be,
                                                             m.scw, m.ptw, m.flag, as, nullptr, m.status);
    else
      k_schnorr_rlc_prep<false><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, cap, in.key, in.sig, in.msgs, in.msg_offsets,
                                                               (uint32_t)in.msg_len, seed_be, m.scw, m.ptw, m.flag, as, nullptr, m.status);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (as_out) *as_out = as;
  if (mode == RLC_PLAIN_TERMS_ONLY) return S2K_OK;
  k_schnorr_rlc_sum<<<RLC_SUM_BLOCKS, 256, 0, st>>>((uint32_t)n, n, as, sum_part, m.scw, m.ptw, m.flag, N, cap, 0u);
  k_schnorr_rlc_sum<<<1, 256, 0, st>>>((uint32_t)n, n, nullptr, sum_part, m.scw, m.ptw, m.flag, N, cap, ecdsa ? 1u : 0u);
  HIP_TRY(ctx, hipGetLastError());
  uint8_t* d_out = (uint8_t*)m.status + 64;   // 65-byte record inside the 256-byte status slot
  rc = msm_core(ctx, st, N, m, d_out, /*affine=*/as_out != nullptr);   // the verdict alone needs no coordinates; the bisection does
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(h, m.status, 64 + 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  return S2K_OK;
}

// the whole-batch verdict of a checked, non-empty batch (the context entered)
static int rlc_verdict(s2k_ctx* ctx, hipStream_t st, size_t n, const rlc_batch& in, const uint8_t* seed32, int* all_valid) {
  msm_ws m;
  uint8_t h[192];
  rlc_key coeff;
  int rc = rlc_run_full(ctx, st, n, in, seed32, m, nullptr, h, RLC_AGGREGATED, coeff, true);
  if (rc) return rc;
  uint32_t h_status;
  memcpy(&h_status, h, 4);
  *all_valid = (h_status == 0 && h[64] == 0x00) ? 1 : 0;
  return S2K_OK;
}

int s2k_schnorr_batch_verify_rlc_device(s2k_ctx* ctx, size_t n, const void* d_pk, const void* d_msgs,
                                        const void* d_msg_offsets, size_t msg_len, const void* d_sig,
                                        const uint8_t* seed32, int* all_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!all_valid || !seed32) return fail(ctx, S2K_ERR_ARG, "null argument");
  *all_valid = 0;
  if (n == 0) {
    *all_valid = 1;   // an empty batch has no failing signature
    return S2K_OK;
  }
  if (!d_pk || !d_sig || (!d_msgs && (d_msg_offsets || msg_len))) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n > 0x0fffffffu || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  return rlc_verdict(ctx, st, n, rlc_batch_bip340(d_pk, d_msgs, d_msg_offsets, msg_len, d_sig), seed32, all_valid);
}

// The kept terms of a batch in the plain form (the context's rlc_save): what a sub-range is gathered from, since the
// sub-range runs re-carve the multiscalar workspace.  `leaf`: leaf_bytes of scratch behind them (the ECDSA leaf verifier's).
struct rlc_saved {
  size_t n;
  uint32_t *scw, *ptw, *as;
  uint8_t *flag, *leaf;
};
static size_t rlc_pad(size_t b) { return (b + 255) & ~(size_t)255; }
// terms, flags and a_i s_i planes of the plain form as rlc_run_full left them in `m` / `as` -> sv
static int rlc_keep_terms(s2k_ctx* ctx, hipStream_t st, size_t n, const msm_ws& m, const uint32_t* as, size_t leaf_bytes, rlc_saved& sv) {
  const size_t NS = 3 * n;
  const size_t o_scw = 0, o_ptw = rlc_pad(NS * (SCW_WORDS - 1) * 4), o_flag = o_ptw + rlc_pad(NS * TERM_REC_WORDS * 4), o_as = o_flag + rlc_pad(n),
               o_leaf = o_as + rlc_pad(n * 8 * 4), total = o_leaf + leaf_bytes;
  int rc = ctx_reserve(ctx, &ctx->rlc_save, &ctx->rlc_save_bytes, total);
  if (rc) return rc;
  uint8_t* base = (uint8_t*)ctx->rlc_save;
  sv.n = n;
  sv.scw = (uint32_t*)(base + o_scw);
  sv.ptw = (uint32_t*)(base + o_ptw);
  sv.as = (uint32_t*)(base + o_as);
  sv.flag = base + o_flag;
  sv.leaf = base + o_leaf;
  k_rlc_save<<<blocks_for(NS), 256, 0, st>>>((uint32_t)n, m.scw, m.ptw, m.flag, sv.scw, sv.ptw, sv.flag);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(sv.as, as, n * 8 * 4, hipMemcpyDeviceToDevice, st));
  return S2K_OK;
}
// error point of the sub-range [lo, lo + cnt) of the kept batch: its 3 cnt terms gathered, its generator term summed, the
// multiscalar core on 3 cnt + 2 terms; E on the host, the stream synchronised
static int rlc_sub_range(s2k_ctx* ctx, hipStream_t st, const rlc_saved& sv, bool ecdsa, uint32_t lo, uint32_t cnt, uint8_t E[65]) {
  msm_ws w;
  const size_t N = 3 * (size_t)cnt + 2;
  int r = msm_setup(ctx, N, 256 + RLC_SUM_BLOCKS * 32, w);
  if (r) return r;
  uint32_t* sum_part = (uint32_t*)w.aux;
  HIP_TRY(ctx, msm_clear(ctx, st, w));
  k_rlc_gather<<<blocks_for(3 * (size_t)cnt), 256, 0, st>>>(lo, cnt, (uint32_t)sv.n, sv.scw, sv.ptw, sv.flag, w.scw, w.ptw, w.flag);
  k_schnorr_rlc_sum<<<RLC_SUM_BLOCKS, 256, 0, st>>>(cnt, sv.n, sv.as + lo, sum_part, w.scw, w.ptw, w.flag, N, N, 0u);
  k_schnorr_rlc_sum<<<1, 256, 0, st>>>(cnt, sv.n, nullptr, sum_part, w.scw, w.ptw, w.flag, N, N, ecdsa ? 1u : 0u);
  HIP_TRY(ctx, hipGetLastError());
  uint8_t* d_out = (uint8_t*)w.status + 64;
  r = msm_core(ctx, st, N, w, d_out);
  if (r) return r;
  HIP_TRY(ctx, hipMemcpyAsync(E, d_out, 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return S2K_OK;
}

// Per-signature verdicts at the price of the whole-batch check when (as usual) everything verifies:
// one combination over the batch; if it is rejected, the failing signatures are located by
// bisection on the kept terms (header).  stats (host, optional): [0] sub-range multiscalar
// multiplications, [1] signatures verified one by one, [2] levels descended, [3] 1 = gave up
// bisecting (many failing ranges) and verified the rest one by one.
// The driver behind both schemes' bisect calls (a checked, non-empty batch; the context entered).
static int rlc_bisect(s2k_ctx* ctx, hipStream_t st, size_t n, const rlc_batch& in, const uint8_t* seed32, uint8_t* valid, uint32_t* stats) {
  const bool ecdsa = in.scheme == RLC_ECDSA;
  int rc;
  // Below LEAF signatures a range is verified signature by signature: a combination costs at least the
  // multiscalar floor (0.75 ms + preparation), per-signature verification 0.56 ms per 2^16 signatures.
  constexpr uint32_t LEAF = 1u << 17;
  constexpr size_t MAX_FAILING = 8;        // more failing ranges than this on one level: stop bisecting
  // The leaf verifier is the ground truth the combination is allowed to skip.  BIP-340: s2k_schnorr_verify_batch.  ECDSA: the
  // keys recovered by s2k_ecdsa_recover_batch_device into `leaf` (65-byte records, then the ok bytes; it lies behind the kept
  // terms in rlc_save, sized for the whole batch: once bisecting is abandoned a range can be any size) and k_ecdsa_rlc_leaf.
  const size_t leaf_bytes = ecdsa ? rlc_pad(n * 65) + rlc_pad(n) : 0;
  uint8_t* leaf = nullptr;
  auto verify_each = [&](uint32_t lo, uint32_t cnt) -> int {
    if (stats) stats[1] += cnt;
    if (!ecdsa)
      return s2k_schnorr_verify_batch_device(ctx, cnt, in.key + (size_t)lo * 32,
                                             in.msg_offsets ? in.msgs : (in.msgs ? in.msgs + (size_t)lo * in.msg_len : nullptr),
                                             in.msg_offsets ? in.msg_offsets + lo : nullptr, in.msg_len, in.sig + (size_t)lo * 64, 0, valid + lo, st);
    uint8_t *rec = leaf, *okb = leaf + rlc_pad(n * 65);
    int r = s2k_ecdsa_recover_batch_device(ctx, cnt, in.dig + (size_t)lo * 32, in.r + (size_t)lo * 32, in.s + (size_t)lo * 32, in.recid + lo,
                                           0u, rec, okb, st);
    if (r) return r;
    k_ecdsa_rlc_leaf<<<blocks_for(cnt), 256, 0, st>>>(cnt, in.key + (size_t)lo * 64, in.s + (size_t)lo * 32, in.flags, rec, okb, valid + lo);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  };
  if (n <= LEAF) {
    if (ecdsa) {
      rc = ctx_reserve(ctx, &ctx->rlc_save, &ctx->rlc_save_bytes, leaf_bytes);
      if (rc) return rc;
      leaf = (uint8_t*)ctx->rlc_save;
    }
    return verify_each(0, (uint32_t)n);
  }

  msm_ws m;
  uint32_t* as = nullptr;
  uint8_t h[192];
  rlc_key coeff;
  rc = rlc_run_full(ctx, st, n, in, seed32, m, &as, h, RLC_AGGREGATED, coeff, true);
  if (rc) return rc;
  if (h[64] == 0x00) {   // the combination of every liftable signature vanishes: those are all valid
    k_rlc_mark_valid<<<blocks_for(n), 256, 0, st>>>(0u, (uint32_t)n, m.flag, valid);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  // Rejected.  The bisection gathers per-signature terms, so the plain form is prepared now, with the
  // coefficients of the pass that has just failed: its error point h + 64 is the plain form's as well.
  {
    uint8_t h2[192];
    rc = rlc_run_full(ctx, st, n, in, seed32, m, &as, h2, RLC_PLAIN_TERMS_ONLY, coeff, false);
    if (rc) return rc;
  }
  // keep the terms: the sub-range runs re-carve the multiscalar workspace
  rlc_saved sv;
  rc = rlc_keep_terms(ctx, st, n, m, as, leaf_bytes, sv);
  if (rc) return rc;
  leaf = sv.leaf;
  const uint8_t* s_flag = sv.flag;

  // error point of a sub-range
  auto sub = [&](uint32_t lo, uint32_t cnt, uint8_t E[65]) -> int {
    int r = rlc_sub_range(ctx, st, sv, ecdsa, lo, cnt, E);
    if (r == S2K_OK && stats) stats[0] += 1;
    return r;
  };
  struct range {
    uint32_t lo, cnt;
    uint8_t E[65];
  };
  std::vector<range> cur(1), next;
  cur[0].lo = 0;
  cur[0].cnt = (uint32_t)n;
  memcpy(cur[0].E, h + 64, 65);
  while (!cur.empty()) {
    if (cur.size() > MAX_FAILING) {   // errors everywhere: bisection would cost more than it saves
      if (stats) stats[3] = 1;
      for (const range& r : cur) {
        rc = verify_each(r.lo, r.cnt);
        if (rc) return rc;
      }
      break;
    }
    next.clear();
    for (const range& r : cur) {
      if (r.cnt <= LEAF) {
        rc = verify_each(r.lo, r.cnt);
        if (rc) return rc;
        continue;
      }
      range left, right;
      left.lo = r.lo;
      left.cnt = r.cnt / 2;
      right.lo = r.lo + left.cnt;
      right.cnt = r.cnt - left.cnt;
      rc = sub(left.lo, left.cnt, left.E);
      if (rc) return rc;
      if (s2k_internal_point_sub65(r.E, left.E, right.E) != 0) return fail(ctx, S2K_ERR_HIP, "internal: bad error point");
      for (const range* h2 : {&left, &right}) {
        if (h2->E[0] == 0x00) {
          k_rlc_mark_valid<<<blocks_for(h2->cnt), 256, 0, st>>>(h2->lo, h2->cnt, s_flag, valid);
          HIP_TRY(ctx, hipGetLastError());
        } else {
          next.push_back(*h2);
        }
      }
    }
    if (stats && !next.empty()) stats[2] += 1;
    cur.swap(next);
  }
  return ctx_leave(ctx, st);
}

int s2k_schnorr_verify_batch_bisect_device(s2k_ctx* ctx, size_t n, const void* d_pk, const void* d_msgs,
                                           const void* d_msg_offsets, size_t msg_len, const void* d_sig,
                                           const uint8_t* seed32, void* d_valid, uint32_t* stats, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!seed32) return fail(ctx, S2K_ERR_ARG, "null argument");
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (n == 0) return S2K_OK;
  if (!d_pk || !d_sig || !d_valid || (!d_msgs && (d_msg_offsets || msg_len))) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n > 0x0fffffffu || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  return rlc_bisect(ctx, st, n, rlc_batch_bip340(d_pk, d_msgs, d_msg_offsets, msg_len, d_sig), seed32, (uint8_t*)d_valid, stats);
}

int s2k_schnorr_verify_batch_bisect(s2k_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* msgs, const uint64_t* msg_offsets,
                                    size_t msg_len, const uint8_t* sig, const uint8_t* seed32, uint8_t* valid, uint32_t* stats) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!pk || !sig || !valid || !seed32) return fail(ctx, S2K_ERR_ARG, "null buffer");
  // before anything is staged: n * msg_len bytes would be reserved and copied from `msgs`
  if (n > 0x0fffffffu || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  uint8_t* d[5];
  hipStream_t st;
  s2k_phase_guard phase(ctx->device, n * 128);           // (two verifiers on two threads: engine_internal.h)
  int rc = stage_schnorr(ctx, n, pk, msgs, msg_offsets, msg_len, sig, d, &st);
  if (rc) return rc;
  HIP_TRY(ctx, phase.landed(st));
  rc = s2k_schnorr_verify_batch_bisect_device(ctx, n, d[0], d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], seed32, d[4], stats, st);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(valid, d[4], n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  return S2K_OK;
}

int s2k_schnorr_batch_verify_rlc(s2k_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* msgs,
                                 const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig,
                                 const uint8_t* seed32, int* all_valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!all_valid || !seed32) return fail(ctx, S2K_ERR_ARG, "null argument");
  *all_valid = 0;       // (a refusal below leaves no verdict of an earlier call behind)
  if (n == 0) {
    *all_valid = 1;
    return S2K_OK;
  }
  if (!pk || !sig) return fail(ctx, S2K_ERR_ARG, "null buffer");
  // before anything is staged: n * msg_len bytes would be reserved and copied from `msgs`
  if (n > 0x0fffffffu || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  uint8_t* d[5];
  hipStream_t st;
  s2k_phase_guard phase(ctx->device, n * 128);           // (two verifiers on two threads: engine_internal.h)
  int rc = stage_schnorr(ctx, n, pk, msgs, msg_offsets, msg_len, sig, d, &st);
  if (rc) return rc;
  HIP_TRY(ctx, phase.landed(st));
  return s2k_schnorr_batch_verify_rlc_device(ctx, n, d[0], d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], seed32, all_valid, st);
}

// ---- recoverable ECDSA signatures (header: the contract; above: k_ecdsa_rlc_prep) ----
// refusals shared by the four entry points: S2K_ERR_ARG before any launch
static int ecdsa_rlc_check_args(s2k_ctx* ctx, size_t n, const void* pub, const void* dig, const void* r, const void* s, const void* recid,
                                uint32_t flags) {
  if (!pub || !dig || !r || !s || !recid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n > 0x0fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  if (flags & ~S2K_ECDSA_REJECT_MALLEABLE) return fail(ctx, S2K_ERR_ARG, "unknown flag bits (S2K_ECDSA_REJECT_MALLEABLE only)");
  return S2K_OK;
}

int s2k_ecdsa_batch_verify_rlc_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r, const void* d_s,
                                      const void* d_recid, uint32_t flags, const uint8_t* seed32, int* all_valid, void* hip_stream) {
  if (all_valid) *all_valid = 0;
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!all_valid || !seed32) return fail(ctx, S2K_ERR_ARG, "null argument");
  int rc = ecdsa_rlc_check_args(ctx, n, d_pub, d_dig, d_r, d_s, d_recid, flags);
  if (rc) return rc;
  if (n == 0) {
    *all_valid = 1;   // an empty batch has no failing item
    return S2K_OK;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  return rlc_verdict(ctx, st, n, rlc_batch_ecdsa(d_pub, d_dig, d_r, d_s, d_recid, flags), seed32, all_valid);
}

int s2k_ecdsa_verify_recoverable_batch_bisect_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r,
                                                     const void* d_s, const void* d_recid, uint32_t flags, const uint8_t* seed32,
                                                     void* d_valid, uint32_t* stats, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!seed32 || !d_valid) return fail(ctx, S2K_ERR_ARG, "null argument");
  int rc = ecdsa_rlc_check_args(ctx, n, d_pub, d_dig, d_r, d_s, d_recid, flags);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (n == 0) return S2K_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  return rlc_bisect(ctx, st, n, rlc_batch_ecdsa(d_pub, d_dig, d_r, d_s, d_recid, flags), seed32, (uint8_t*)d_valid, stats);
}

// stage (pub, digest, r, s, recovery id [, valid]) of a batch in the context's buffers on its compute stream
static int stage_ecdsa_rlc(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                           const uint8_t* recid, uint8_t* d[6], hipStream_t* st_out) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  const size_t sizes[6] = {n * 64, n * 32, n * 32, n * 32, n, n};
  rc = ctx_stage(ctx, sizes, 6, d);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  const uint8_t* src[5] = {pub, dig, r, s, recid};
  for (int k = 0; k < 5; ++k) HIP_TRY(ctx, hipMemcpyAsync(d[k], src[k], sizes[k], hipMemcpyHostToDevice, st));
  *st_out = st;
  return S2K_OK;
}

int s2k_ecdsa_batch_verify_rlc(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                               const uint8_t* recid, uint32_t flags, const uint8_t* seed32, int* all_valid) {
  if (all_valid) *all_valid = 0;
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!all_valid || !seed32) return fail(ctx, S2K_ERR_ARG, "null argument");
  int rc = ecdsa_rlc_check_args(ctx, n, pub, dig, r, s, recid, flags);
  if (rc) return rc;
  if (n == 0) {
    *all_valid = 1;
    return S2K_OK;
  }
  uint8_t* d[6];
  hipStream_t st;
  s2k_phase_guard phase(ctx->device, n * 161);           // (two verifiers on two threads: engine_internal.h)
  rc = stage_ecdsa_rlc(ctx, n, pub, dig, r, s, recid, d, &st);
  if (rc) return rc;
  HIP_TRY(ctx, phase.landed(st));
  return s2k_ecdsa_batch_verify_rlc_device(ctx, n, d[0], d[1], d[2], d[3], d[4], flags, seed32, all_valid, st);
}

int s2k_ecdsa_verify_recoverable_batch_bisect(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                              const uint8_t* s, const uint8_t* recid, uint32_t flags, const uint8_t* seed32,
                                              uint8_t* valid, uint32_t* stats) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!seed32 || !valid) return fail(ctx, S2K_ERR_ARG, "null argument");
  int rc = ecdsa_rlc_check_args(ctx, n, pub, dig, r, s, recid, flags);
  if (rc) return rc;
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (n == 0) return S2K_OK;
  uint8_t* d[6];
  hipStream_t st;
  s2k_phase_guard phase(ctx->device, n * 161);           // (two verifiers on two threads: engine_internal.h)
  rc = stage_ecdsa_rlc(ctx, n, pub, dig, r, s, recid, d, &st);
  if (rc) return rc;
  HIP_TRY(ctx, phase.landed(st));
  rc = s2k_ecdsa_verify_recoverable_batch_bisect_device(ctx, n, d[0], d[1], d[2], d[3], d[4], flags, seed32, d[5], stats, st);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(valid, d[5], n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  return S2K_OK;
}

// ---- test hooks: the error point of a whole-batch check under a GIVEN coefficient key (see the header) ----
// (a staged, checked batch; the context entered).  form 0: what rlc_verdict runs, with the affine record of the bisect call's
// first pass; form 1: the plain-form terms kept and the sub-range [lo, lo + cnt) summed, by the functions rlc_bisect runs.
static int rlc_debug_point(s2k_ctx* ctx, hipStream_t st, size_t n, const rlc_batch& in, const uint8_t* key32, int form, size_t lo,
                           size_t cnt, uint8_t* out65, uint32_t* status, uint8_t* in_comb) {
  rlc_key coeff;
  for (int j = 0; j < 8; ++j)
    coeff.w[j] = ((uint32_t)key32[4 * j] << 24) | ((uint32_t)key32[4 * j + 1] << 16) | ((uint32_t)key32[4 * j + 2] << 8) | key32[4 * j + 3];
  msm_ws m;
  uint32_t* as = nullptr;
  uint8_t h[192];
  const uint8_t* d_flag;
  if (form == 0) {
    int rc = rlc_run_full(ctx, st, n, in, key32, m, &as, h, RLC_AGGREGATED, coeff, false);
    if (rc) return rc;
    memcpy(status, h, 4);
    memcpy(out65, h + 64, 65);
    d_flag = m.flag;
  } else {
    int rc = rlc_run_full(ctx, st, n, in, key32, m, &as, h, RLC_PLAIN_TERMS_ONLY, coeff, false);
    if (rc) return rc;
    // the preparation's word, over the whole batch: the sub-range step re-carves the workspace and zeroes it
    HIP_TRY(ctx, hipMemcpyAsync(status, m.status, 4, hipMemcpyDeviceToHost, st));
    rlc_saved sv;
    rc = rlc_keep_terms(ctx, st, n, m, as, 0, sv);
    if (rc) return rc;
    rc = rlc_sub_range(ctx, st, sv, in.scheme == RLC_ECDSA, (uint32_t)lo, (uint32_t)cnt, out65);
    if (rc) return rc;
    d_flag = sv.flag;
  }
  if (in_comb) HIP_TRY(ctx, hipMemcpyAsync(in_comb, d_flag, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return S2K_OK;
}
static int rlc_debug_check_args(s2k_ctx* ctx, size_t n, const void* key32, int form, size_t lo, size_t cnt, const void* out65,
                                const void* status) {
  if (!key32 || !out65 || !status) return fail(ctx, S2K_ERR_ARG, "null argument");
  if (n == 0 || n > MSM_DEBUG_TERMS_MAX) return fail(ctx, S2K_ERR_ARG, "batch size outside 1 .. 2^22");
  if (form != 0 && form != 1) return fail(ctx, S2K_ERR_ARG, "form must be 0 (aggregated) or 1 (plain, sub-range)");
  if (form == 0 ? (lo != 0 || cnt != n) : (cnt == 0 || lo >= n || cnt > n - lo))
    return fail(ctx, S2K_ERR_ARG, "range outside the batch (the aggregated form takes the whole batch only)");
  return S2K_OK;
}
// enter, run, leave: every path behind ctx_enter goes through ctx_leave, a failed one with nothing left in flight
static int rlc_debug_run(s2k_ctx* ctx, hipStream_t st, size_t n, const rlc_batch& in, const uint8_t* key32, int form, size_t lo,
                         size_t cnt, uint8_t* out65, uint32_t* status, uint8_t* in_comb) {
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = rlc_debug_point(ctx, st, n, in, key32, form, lo, cnt, out65, status, in_comb);
  if (rc) s2k_internal_drain(ctx);
  const int left = ctx_leave(ctx, st);
  if (rc == S2K_OK && left == S2K_OK) ctx->have_last = false;   // the stream has been synchronised
  return rc ? rc : left;
}

int s2k_debug_schnorr_rlc_point(s2k_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* msgs, const uint64_t* msg_offsets, size_t msg_len,
                                const uint8_t* sig, const uint8_t* key32, int form, size_t lo, size_t cnt, uint8_t* out65,
                                uint32_t* status, uint8_t* in_comb) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!pk || !sig) return fail(ctx, S2K_ERR_ARG, "null buffer");
  int rc = rlc_debug_check_args(ctx, n, key32, form, lo, cnt, out65, status);
  if (rc) return rc;
  if (msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());               // nothing in flight reads the buffers below
  uint8_t* d[5];
  hipStream_t st;
  rc = stage_schnorr(ctx, n, pk, msgs, msg_offsets, msg_len, sig, d, &st);
  if (rc) {
    s2k_internal_drain(ctx);
    return rc;
  }
  return rlc_debug_run(ctx, st, n, rlc_batch_bip340(d[0], d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3]), key32, form, lo, cnt,
                       out65, status, in_comb);
}

int s2k_debug_ecdsa_rlc_point(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                              const uint8_t* recid, uint32_t flags, const uint8_t* key32, int form, size_t lo, size_t cnt,
                              uint8_t* out65, uint32_t* status, uint8_t* in_comb) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = ecdsa_rlc_check_args(ctx, n, pub, dig, r, s, recid, flags);
  if (rc) return rc;
  rc = rlc_debug_check_args(ctx, n, key32, form, lo, cnt, out65, status);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());               // nothing in flight reads the buffers below
  uint8_t* d[6];
  hipStream_t st;
  rc = stage_ecdsa_rlc(ctx, n, pub, dig, r, s, recid, d, &st);
  if (rc) {
    s2k_internal_drain(ctx);
    return rc;
  }
  return rlc_debug_run(ctx, st, n, rlc_batch_ecdsa(d[0], d[1], d[2], d[3], d[4], flags), key32, form, lo, cnt, out65, status, in_comb);
}

}  // extern "C"
