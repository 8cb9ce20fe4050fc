// small_call.hip — the kernels of calls too small to fill the chip with one lane per signature, and their launchers
// (engine_internal.h): one WAVEFRONT per signature (k_verify_row, k_schnorr_row, k_recover_row, and k_verify_row_keyset /
// _comb, k_schnorr_row_keyset / _comb over a key set's tables) and FOUR LANES per signature (k_verify_quad, k_schnorr_quad,
// k_recover_quad).  The flows that choose them are engine.hip's and keyset.hip's; the one-lane preparation their fifth waves
// run is sig_prep.h's; the row and quad arithmetic fe29r.h's and pt29q.h's.
//
// Several bodies here are near copies on purpose: the generator-table tail of row_ladder / row_ladder_keyset / row_ladder_comb,
// the ECDSA accept rule of the three k_verify_row* kernels, k_verify_row_keyset against _comb, k_schnorr_row_keyset against
// _comb, and the common prefix of fer_sqrt_chain / fer_inv_chain.  Sharing them was tried when this unit was split off: a
// common generator tail moved four opcode positions in each of the six row kernels, a common verdict made the three ECDSA row
// kernels one instruction shorter.  Small as that is, it is other machine code, so it wants an A/B on the device, not a move.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "sig_prep.h"
#include "fe.h"
#include "lane_tables.h"
#include "pt29.h"
#include "fe29r.h"
#include "pt29q.h"
#include "complete_path.h"
#include "point.h"
#include "sc.h"

using namespace s2k;

// ---------------------------------------------------------------------------------------
// Small batches: ONE WAVE PER SIGNATURE (round 5).  A call of up to a few thousand signatures - the reference's own
// shape is a loop of single Verify calls, BASELINE config 1 verifies 1024 - leaves the chip empty whatever the kernel: what
// it costs is the latency of one lane's ladder, 261 k dependent instructions, 0.7 ms for 64 signatures as for 8192
// (bench.py batch_sweep).  Here the ladder runs in the row arithmetic of fe29r.h (a field element = one register, one limb
// per lane of a 16-lane row, the four products of a formula layer in the four rows of the wave): the same signed-odd-digit
// GLV ladder as k_verify_fast - table {1,3,..,15} Q, 32 windows of four doublings and two additions, the generator part from
// the resident tables - on the COMPLETE projective formulas (pt29r_add / pt29r_double: no exceptional case, so no worklist
// and no second kernel), ~70 k instructions of one wave per signature.  Digits, table indices and generator-table addresses
// are wave-uniform.  Verdicts are those of the other paths (same preparation kernel, same accept rule ecdsa.go:392-470).
// ---------------------------------------------------------------------------------------
// limb j (lane j of every row) of a 256-bit value given as eight little-endian words every lane holds
S2K_DEV fer fer_from_words(const uint32_t w[8], const fer_consts& k) {
  const uint32_t bit = 29u * k.j, idx = bit >> 5, sh = bit & 31u;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    lo = idx == (uint32_t)i ? w[i] : lo;
    hi = idx + 1 == (uint32_t)i ? w[i] : hi;
  }
  const uint64_t v = ((uint64_t)hi << 32) | lo;
  return k.j <= 8 ? ((uint32_t)(v >> sh) & F29_M) : 0u;       // (limb 8: bits 232..255, 24 of them)
}
// value == 0 (mod p), the same answer in every lane
S2K_DEV bool fer_is_zero(fer a, const fer_consts& k) { return fe29_is_zero(fer_to_fe29(fer_norm(a, k))); }

// canonical value odd?  (the same answer in every lane of a row)
S2K_DEV bool fer_is_odd(fer a, const fer_consts& k) { return (fe29_normalize(fer_to_fe29(fer_norm(a, k))).n[0] & 1u) != 0; }
S2K_DEV fer fer_sqr_n(fer a, int n, const fer_consts& k) {
#pragma unroll 1
  for (int i = 0; i < n; ++i) a = fer_mul(a, a, k);
  return a;
}
// a^((p+1)/4): the chain of fe29_sqrt (Sqrt, internal/field/field_sqrt_ratio.go:14), row by row - four roots per wave
S2K_DEV fer fer_sqrt_chain(fer a, const fer_consts& k) {
  const fer x2 = fer_mul(fer_mul(a, a, k), a, k);
  const fer x3 = fer_mul(fer_mul(x2, x2, k), a, k);
  const fer x6 = fer_mul(fer_sqr_n(x3, 3, k), x3, k);
  const fer x9 = fer_mul(fer_sqr_n(x6, 3, k), x3, k);
  const fer x11 = fer_mul(fer_sqr_n(x9, 2, k), x2, k);
  const fer x22 = fer_mul(fer_sqr_n(x11, 11, k), x11, k);
  const fer x44 = fer_mul(fer_sqr_n(x22, 22, k), x22, k);
  const fer x88 = fer_mul(fer_sqr_n(x44, 44, k), x44, k);
  const fer x176 = fer_mul(fer_sqr_n(x88, 88, k), x88, k);
  const fer x220 = fer_mul(fer_sqr_n(x176, 44, k), x44, k);
  const fer x223 = fer_mul(fer_sqr_n(x220, 3, k), x3, k);
  fer t = fer_mul(fer_sqr_n(x223, 23, k), x22, k);
  t = fer_mul(fer_sqr_n(t, 6, k), x2, k);
  return fer_sqr_n(t, 2, k);
}
// x^3 + 7
S2K_DEV fer fer_curve_rhs(fer x, const fer_consts& k) {
  const fer seven = k.j == 0 ? 7u : 0u;
  return fer_mul_plus(fer_mul(x, x, k), x, seven, k);
}

// The wave-per-signature kernels.  A block is four signature waves and one PREPARATION wave: lanes 0..3 of the
// fifth wave run the scalar arithmetic of the block's four signatures (s^-1, u1, u2, the odd GLV split: one lane's chain of
// 55 us) into LDS while the signature waves do what does not depend on it - key checks, square roots, the key's table -, then
// the block meets at one barrier.  One launch per call.
//
// row_table: the table of the key in LDS, one 256-byte line per coordinate of an entry (lane l of the wave at word l) - x, y,
// z and lambda's x (beta * x) of (2j + 1) Q, j < 8; an entry is three loads at a wave-uniform offset.
S2K_DEV void row_table(const pt29r& Q1, uint32_t (*tab)[8][64], const fer_consts& k, uint32_t lane) {
  const fer beta = fer_from_words(FE_BETA, k);
  const pt29r D = pt29r_double(Q1, k);
  pt29r cur = Q1;
#pragma unroll 1
  for (int j = 0; j < 8; ++j) {
    if (j) cur = pt29r_add(cur, D, k);
    tab[0][j][lane] = cur.x;
    tab[1][j][lane] = fer_norm(cur.y, k);
    tab[2][j][lane] = cur.z;
    tab[3][j][lane] = fer_mul(cur.x, beta, k);
  }
}
// u * G + k1 * Q + k2 * lambda(Q) for ONE signature on the whole wave, Q's table in `tab`, u | k1 | k2 | flags in the 17 words
// `p` (LDS): 32 x (4 doublings + 2 additions) on the complete formulas, then the generator part from the resident tables (no
// entry is the identity, no digit is special).  The result is projective.
S2K_DEV pt29r row_ladder(uint32_t (*tab)[8][64], const uint32_t* p, gt_view gt, const fer_consts& k, uint32_t lane) {
  const fer one = k.j == 0 ? 1u : 0u;
  const uint32_t pf = p[16];
  // |k1|, |k2| odd, < 2^129 (sc_split_glv_odd)
  sc k1 = sc_zero(), k2 = sc_zero();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    k1.v[w] = p[8 + w];
    k2.v[w] = p[12 + w];
  }
  k1.v[4] = (pf & PF_K1_B128) ? 1u : 0u;
  k2.v[4] = (pf & PF_K2_B128) ? 1u : 0u;
  const bool neg1 = pf & PF_NEG1, neg2 = pf & PF_NEG2;
  digit_stream d1 = ds_init(k1), d2 = ds_init(k2);
  auto entry_of = [&](uint32_t w, bool lam, bool sneg) -> pt29r {   // the entry of digit w (signed odd: 2w - 15), or its image
    const bool neg = sneg != (w < 8u);                              // under the endomorphism, negated with the scalar's sign
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)((w < 8u) ? (7u - w) : (w - 8u)));
    pt29r a;
    a.x = tab[lam ? 3 : 0][e][lane];
    a.y = tab[1][e][lane];
    a.z = tab[2][e][lane];
    if (neg) a.y = fer_negate(a.y, 1, k);                           // [2]: the addition normalises y
    return a;
  };
  pt29r acc = pt29r_add(entry_of(8u, false, neg1), entry_of(8u, true, neg2), k);   // the top digits are +1 (w = 8)
#pragma unroll 1
  for (int i = 31; i >= 0; --i) {
    const uint32_t w1 = ds_next(d1), w2 = ds_next(d2);
    const pt29r a1 = entry_of(w1, false, neg1), a2 = entry_of(w2, true, neg2);   // (in flight during the doublings)
#pragma unroll 1
    for (int j = 0; j < 4; ++j) acc = pt29r_double(acc, k);
    acc = pt29r_add(acc, a1, k);
    acc = pt29r_add(acc, a2, k);
  }
  uint32_t u[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) u[w] = p[w];
  apt g = gt_load(gt, 0, gt_next_digit(u, gt.bits));
#pragma unroll 1
  for (uint32_t w = 0; w < gt.windows; ++w) {
    pt29r q;
    q.x = fer_from_words(g.x.v, k);
    q.y = fer_from_words(g.y.v, k);
    q.z = one;
    if (w + 1 < gt.windows) g = gt_load(gt, w + 1, gt_next_digit(u, gt.bits));   // in flight during the addition
    acc = pt29r_add(acc, q, k);
  }
  return acc;
}
// a^(p-2), the chain of fe29_inv (Invert, internal/field/field_invert.go:11), in row products
S2K_DEV fer fer_inv_chain(fer a, const fer_consts& k) {
  const fer x2 = fer_mul(fer_mul(a, a, k), a, k);
  const fer x3 = fer_mul(fer_mul(x2, x2, k), a, k);
  const fer x6 = fer_mul(fer_sqr_n(x3, 3, k), x3, k);
  const fer x9 = fer_mul(fer_sqr_n(x6, 3, k), x3, k);
  const fer x11 = fer_mul(fer_sqr_n(x9, 2, k), x2, k);
  const fer x22 = fer_mul(fer_sqr_n(x11, 11, k), x11, k);
  const fer x44 = fer_mul(fer_sqr_n(x22, 22, k), x22, k);
  const fer x88 = fer_mul(fer_sqr_n(x44, 44, k), x44, k);
  const fer x176 = fer_mul(fer_sqr_n(x88, 88, k), x88, k);
  const fer x220 = fer_mul(fer_sqr_n(x176, 44, k), x44, k);
  const fer x223 = fer_mul(fer_sqr_n(x220, 3, k), x3, k);
  fer t = fer_mul(fer_sqr_n(x223, 23, k), x22, k);
  t = fer_mul(fer_sqr_n(t, 5, k), a, k);
  t = fer_mul(fer_sqr_n(t, 3, k), x2, k);
  return fer_mul(fer_sqr_n(t, 2, k), a, k);
}

// PublicKey.Verify (secec/ecdsa.go:171, 392-470) with one WAVEFRONT per signature: the small-batch ladder
__global__ void __launch_bounds__(320)
k_verify_row(uint32_t n, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig,
             const uint8_t* __restrict__ ssig, uint32_t flags, gt_view gt, uint8_t* __restrict__ out) {
  __shared__ uint32_t tab_all[4][4][8][64];
  __shared__ uint32_t prep_s[4][20];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wave == 4) {                                              // the preparation wave
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) scalar_prep_one(i, dig, rsig, ssig, nullptr, flags, prep_s[lane]);
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  const fer_consts k = fer_setup(lane);
  bool ok = sig < n;
  if (ok) {
    uint32_t xw[8], yw[8];
    load_be32(xw, pub + (size_t)sig * 64);
    load_be32(yw, pub + (size_t)sig * 64 + 32);
    ok = fe_is_canonical_raw(xw) && fe_is_canonical_raw(yw);
    pt29r Q1;
    Q1.x = fer_from_words(xw, k);
    Q1.y = fer_from_words(yw, k);
    Q1.z = k.j == 0 ? 1u : 0u;
    // y^2 == x^3 + 7 (point_s11n.go:298-307)
    ok = ok && fer_is_zero(fer_add(fer_mul(Q1.y, Q1.y, k), fer_negate(fer_curve_rhs(Q1.x, k), 1, k)), k);
    if (ok) row_table(Q1, tab_all[wave], k, lane);              // (wave-uniform)
  }
  __syncthreads();
  if (sig >= n) return;
  const uint32_t* p = prep_s[wave];
  if (!(ok && (p[16] & PF_OK))) {
    if (lane == 0) out[sig] = 0;
    return;
  }
  const pt29r acc = row_ladder(tab_all[wave], p, gt, k, lane);
  // ---- verdict: R != infinity and x(R) mod n == r (ecdsa.go:450-465), x(R) = X / Z ----
  uint8_t verdict = 0;
  if (!fer_is_zero(acc.z, k)) {
    uint32_t rw[8];
    load_be32(rw, rsig + (size_t)sig * 32);
    bool match = fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(fer_from_words(rw, k), acc.z, k), 1, k)), k);
    if (u256_lt(rw, FE_P_MINUS_N)) {
      uint32_t r2[8];
      u256_add(r2, rw, SC_N);
      match = match || fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(fer_from_words(r2, k), acc.z, k), 1, k)), k);
    }
    verdict = match ? 1 : 0;
  }
  if (lane == 0) out[sig] = verdict;
}

// ---- small calls over a KEY SET: the wave-per-signature ladder on the set's 32-chunk tables ----
// Every layout but the comb keeps {1,3,..,15} 16^c Q, c < 32, and the lead pair L +- phi(L), L = 16^32 Q, per key
// (kt_geom<32>): the key part of a signature is 64 table additions, no doubling, no table build, no curve check.  The entries
// are AFFINE points of the key's isomorphic curve y^2 = x^3 + 7 W^6 (one shared Z = W per key, keyed.hip), and the complete
// addition contains the curve constant: pt29r_add_b3 with b3 = 21 W^6, formed once per signature.  The sum goes back to
// secp256k1 by pt29r_from_iso and takes the generator part as row_ladder does.
// limb j (lane j of every row) of element `which` (0: x, 1: y, 2: beta x) of the 128-byte entry at e (lane_tables.h: ke_store3)
S2K_DEV fer ke_row_load(const uint4* __restrict__ e, uint32_t which, const fer_consts& k) {
  const uint32_t v = reinterpret_cast<const uint32_t*>(e)[k.j < 8 ? which * 8u + k.j : 24u + which];   // (lanes 9..15: limb 8's word)
  return k.j <= 8 ? v : 0u;
}
struct row_iso {       // of the signature's key: W, W^3, 21 W^6
  fer w, w3, b3;
};
S2K_DEV row_iso row_iso_of(const uint4* __restrict__ kt, const fer_consts& k) {
  using G = kt_geom<KS_CHUNKS>;
  row_iso r;
  r.w = ke_row_load(kt + (size_t)(G::SCR + G::W_SLOT / 3) * 8, G::W_SLOT % 3, k);
  r.w3 = fer_mul(fer_mul(r.w, r.w, k), r.w, k);
  r.b3 = fer_small_norm(fer_mul(r.w3, r.w3, k), 21u, k);
  return r;
}
// u * G + (+-k1) * Q + (+-k2) * lambda(Q), Q the key of table kt: u | k1 | k2 | flags in the 17 words `p` (LDS), the digits those
// of k_verify_fast<MODE_ECDSA_KEYSET> (nibble c of (k - 1) / 2 selects +-(2j + 1) 16^c Q, the lead pair first).  `flip`
// changes both signs (BIP-340 over a key stored with odd Y).  Digits and addresses are wave-uniform; the result is projective.
S2K_DEV pt29r row_ladder_keyset(const uint4* __restrict__ kt, const row_iso& iso, const uint32_t* p, bool flip, gt_view gt,
                                const fer_consts& k) {
  using G = kt_geom<KS_CHUNKS>;
  const fer one = k.j == 0 ? 1u : 0u;
  const uint32_t pf = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[16]);
  const bool neg1 = ((pf & PF_NEG1) != 0) != flip, neg2 = ((pf & PF_NEG2) != 0) != flip;
  uint32_t a[4], b[4];       // (k1 - 1) / 2, (k2 - 1) / 2: 128 bits each
  {
    uint32_t k1[5], k2[5];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      k1[w] = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[8 + w]);
      k2[w] = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[12 + w]);
    }
    k1[4] = (pf & PF_K1_B128) ? 1u : 0u;
    k2[4] = (pf & PF_K2_B128) ? 1u : 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      a[w] = (k1[w] >> 1) | (k1[w + 1] << 31);
      b[w] = (k2[w] >> 1) | (k2[w + 1] << 31);
    }
  }
  auto entry_of = [&](uint32_t c, uint32_t w, bool lam, bool sneg) -> pt29r {   // digit w (signed odd: 2w - 15) of chunk c
    const bool neg = sneg != (w < 8u);
    const uint4* e = kt + (size_t)(c * 8u + ((w < 8u) ? (7u - w) : (w - 8u))) * 8;
    pt29r r;
    r.x = ke_row_load(e, lam ? 2u : 0u, k);
    r.y = ke_row_load(e, 1u, k);
    r.z = one;
    if (neg) r.y = fer_negate(r.y, 1, k);                           // [2]: the addition normalises y
    return r;
  };
  pt29r acc;
  {
    const uint4* e = kt + (size_t)(neg1 == neg2 ? G::LEAD : G::LEAD + 1) * 8;   // +-(L +- phi(L))
    acc.x = ke_row_load(e, 0u, k);
    acc.y = ke_row_load(e, 1u, k);
    acc.z = one;
    if (neg1) acc.y = fer_negate(acc.y, 1, k);
  }
  pt29r a1 = entry_of(0u, a[0] & 15u, false, neg1), a2 = entry_of(0u, b[0] & 15u, true, neg2);
#pragma unroll 1
  for (uint32_t c = 0; c < (uint32_t)KS_CHUNKS; ++c) {
    const pt29r c1 = a1, c2 = a2;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      a[w] = (a[w] >> 4) | (a[w + 1] << 28);
      b[w] = (b[w] >> 4) | (b[w + 1] << 28);
    }
    a[3] >>= 4;
    b[3] >>= 4;
    if (c + 1 < (uint32_t)KS_CHUNKS) {                              // in flight during the additions
      a1 = entry_of(c + 1, a[0] & 15u, false, neg1);
      a2 = entry_of(c + 1, b[0] & 15u, true, neg2);
    }
    acc = pt29r_add_b3(acc, c1, iso.b3, k);
    acc = pt29r_add_b3(acc, c2, iso.b3, k);
  }
  acc = pt29r_from_iso(acc, iso.w, iso.w3, k);
  uint32_t u[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) u[w] = p[w];
  apt g = gt_load(gt, 0, gt_next_digit(u, gt.bits));
#pragma unroll 1
  for (uint32_t w = 0; w < gt.windows; ++w) {
    pt29r q;
    q.x = fer_from_words(g.x.v, k);
    q.y = fer_from_words(g.y.v, k);
    q.z = one;
    if (w + 1 < gt.windows) g = gt_load(gt, w + 1, gt_next_digit(u, gt.bits));   // in flight during the addition
    acc = pt29r_add(acc, q, k);
  }
  return acc;
}

// k_verify_row over a key set: the signature names its key by index; an index outside the set or a key the set marks invalid
// gives 0 without touching a table.  The block's preparation wave is the critical path in front of the ladder here (there is
// no table build to hide it behind); the signature waves form W^3 and 21 W^6 meanwhile.
__global__ void __launch_bounds__(320)
k_verify_row_keyset(uint32_t n, uint32_t nkeys, const uint32_t* __restrict__ kidx, const uint4* __restrict__ ktab,
                    const uint8_t* __restrict__ tinfo, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig,
                    const uint8_t* __restrict__ ssig, uint32_t flags, gt_view gt, uint8_t* __restrict__ out) {
  __shared__ uint32_t prep_s[4][20];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wave == 4) {                                              // the preparation wave
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) scalar_prep_one(i, dig, rsig, ssig, nullptr, flags, prep_s[lane]);
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  const fer_consts k = fer_setup(lane);
  bool ok = false;
  const uint4* kt = ktab;
  row_iso iso = {0u, 0u, 0u};
  if (sig < n) {
    const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)kidx[sig]);
    ok = key < nkeys && tinfo[key < nkeys ? key : 0u] != 0;
    if (ok) {                                                   // (wave-uniform)
      kt = ktab + (size_t)key * (KS_SLOTS * 8);
      iso = row_iso_of(kt, k);
    }
  }
  __syncthreads();
  if (sig >= n) return;
  const uint32_t* p = prep_s[wave];
  if (!(ok && (p[16] & PF_OK))) {
    if (lane == 0) out[sig] = 0;
    return;
  }
  const pt29r acc = row_ladder_keyset(kt, iso, p, false, gt, k);
  // ---- verdict: R != infinity and x(R) mod n == r (ecdsa.go:450-465), x(R) = X / Z ----
  uint8_t verdict = 0;
  if (!fer_is_zero(acc.z, k)) {
    uint32_t rw[8];
    load_be32(rw, rsig + (size_t)sig * 32);
    bool match = fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(fer_from_words(rw, k), acc.z, k), 1, k)), k);
    if (u256_lt(rw, FE_P_MINUS_N)) {
      uint32_t r2[8];
      u256_add(r2, rw, SC_N);
      match = match || fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(fer_from_words(r2, k), acc.z, k), 1, k)), k);
    }
    verdict = match ? 1 : 0;
  }
  if (lane == 0) out[sig] = verdict;
}

// ---- small calls over a COMB key set (S2K_KEYSET_COMB) ----
// The comb's ladder doubles, and a doubling on the key's isomorphic curve would need the per-key constant as the addition
// there does.  It is not run there: an affine entry (x, y) of y^2 = x^3 + 7 W^6 IS the projective point (x W : y : W^3) of
// secp256k1 (pt29r_pair_from_iso, fe29r.h: one layer for the two entries of a column), and from then on the ladder is
// pt29r_double and pt29r_add on secp256k1 itself - no b3, and no map back at the end.  37 additions of 3 layers, 18 doublings
// of 2 and 19 conversions: 166 row-product layers on the key part, where row_ladder_keyset spends 64 x 4 + 1.
// The key's W (one unit: a product's output) and W^3, formed once per signature
struct row_comb_iso {
  fer w, w3;
};
S2K_DEV row_comb_iso row_comb_iso_of(const uint4* __restrict__ kt, const fer_consts& k) {
  row_comb_iso r;
  r.w = ke_row_load(kt + (size_t)kc_geom::WENT * 8, kc_geom::W, k);
  r.w3 = fer_mul(fer_mul(r.w, r.w, k), r.w, k);
  return r;
}
// u * G + (+-k1) * Q + (+-k2) * lambda(Q), Q the key of the comb table kt (kc_geom): u | k1 | k2 | flags in the 17 words `p`
// (LDS), the recoding that of k_verify_comb (comb_ladder.hip) - a' = (k >> 1) | 2^132 per half, tooth t its bits 19 t ..
// 19 t + 18, column j the 7-bit index whose top bit is the sign; the LEAD slots are not read.  Column 18 starts the
// accumulator as the sum of its two entries; rounds 17..0 double, add E1, add phi(E2).  `flip` changes both signs (BIP-340
// over a key stored with odd Y).  Teeth, indices, signs and addresses are wave-uniform; the result is projective.
S2K_DEV pt29r row_ladder_comb(const uint4* __restrict__ kt, fer w, fer w3, const uint32_t* p, bool flip, gt_view gt, const fer_consts& k) {
  using G = kc_geom;
  const fer one = k.j == 0 ? 1u : 0u;
  const uint32_t pf = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[16]);
  const bool neg1 = ((pf & PF_NEG1) != 0) != flip, neg2 = ((pf & PF_NEG2) != 0) != flip;
  uint32_t t1[G::TEETH], t2[G::TEETH];
  {
    uint32_t k1[5], k2[5];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      k1[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[8 + i]);
      k2[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)p[12 + i]);
    }
    k1[4] = (pf & PF_K1_B128) ? 1u : 0u;
    k2[4] = (pf & PF_K2_B128) ? 1u : 0u;
#pragma unroll
    for (int t = 0; t < G::TEETH; ++t) {
      const int bit = G::SPACING * t + 1, limb = bit >> 5, sh = bit & 31;      // (+ 1: a = k >> 1)
      uint32_t v1 = k1[limb] >> sh, v2 = k2[limb] >> sh;
      if (sh > 32 - G::SPACING) {
        v1 |= k1[limb + 1] << (32 - sh);
        v2 |= k2[limb + 1] << (32 - sh);
      }
      t1[t] = v1 & ((1u << G::SPACING) - 1u);
      t2[t] = v2 & ((1u << G::SPACING) - 1u);
    }
    t1[G::TEETH - 1] |= 1u << (G::SPACING - 1);                                 // a' = a | 2^132: the lead, as a digit
    t2[G::TEETH - 1] |= 1u << (G::SPACING - 1);
  }
  struct column {       // the two entries of a column as loaded: x of E1, beta x of E2, their y and whether each is negated
    fer x1, y1, x2, y2;
    bool n1, n2;
  };
  auto fetch = [&](int j) -> column {
    uint32_t w1 = 0, w2 = 0;
#pragma unroll
    for (int t = 0; t < G::TEETH; ++t) {
      w1 |= ((t1[t] >> j) & 1u) << t;
      w2 |= ((t2[t] >> j) & 1u) << t;
    }
    const bool top1 = (w1 & 64u) != 0, top2 = (w2 & 64u) != 0;
    const uint4 *e1 = kt + (size_t)((top1 ? w1 : ~w1) & 63u) * 8, *e2 = kt + (size_t)((top2 ? w2 : ~w2) & 63u) * 8;
    column c;
    c.x1 = ke_row_load(e1, 0u, k);
    c.y1 = ke_row_load(e1, 1u, k);
    c.x2 = ke_row_load(e2, 2u, k);
    c.y2 = ke_row_load(e2, 1u, k);
    c.n1 = neg1 != !top1;
    c.n2 = neg2 != !top2;
    return c;
  };
  auto entries = [&](const column& c, pt29r& e1, pt29r& e2) {
    pt29r_pair_from_iso(c.x1, c.n1 ? fer_negate(c.y1, 1, k) : c.y1, c.x2, c.n2 ? fer_negate(c.y2, 1, k) : c.y2, w, w3, e1, e2, k);   // y [2]
  };
  column nx = fetch(G::SPACING - 1);
  pt29r acc, e1, e2;
  {
    const column c = nx;
    nx = fetch(G::SPACING - 2);                                     // in flight during the addition
    entries(c, e1, e2);
    acc = pt29r_add(e1, e2, k);
  }
#pragma unroll 1
  for (int j = G::SPACING - 2; j >= 0; --j) {
    const column c = nx;
    if (j > 0) nx = fetch(j - 1);                                   // in flight during the round
    acc = pt29r_double(acc, k);
    entries(c, e1, e2);
    acc = pt29r_add(acc, e1, k);
    acc = pt29r_add(acc, e2, k);
  }
  uint32_t u[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) u[i] = p[i];
  apt g = gt_load(gt, 0, gt_next_digit(u, gt.bits));
#pragma unroll 1
  for (uint32_t i = 0; i < gt.windows; ++i) {
    pt29r q;
    q.x = fer_from_words(g.x.v, k);
    q.y = fer_from_words(g.y.v, k);
    q.z = one;
    if (i + 1 < gt.windows) g = gt_load(gt, i + 1, gt_next_digit(u, gt.bits));   // in flight during the addition
    acc = pt29r_add(acc, q, k);
  }
  return acc;
}

// k_verify_row_keyset over a comb set: same block, same validity rules, the table stride is the comb's
__global__ void __launch_bounds__(320)
k_verify_row_comb(uint32_t n, uint32_t nkeys, const uint32_t* __restrict__ kidx, const uint4* __restrict__ ktab,
                  const uint8_t* __restrict__ tinfo, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig,
                  const uint8_t* __restrict__ ssig, uint32_t flags, gt_view gt, uint8_t* __restrict__ out) {
  __shared__ uint32_t prep_s[4][20];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wave == 4) {                                              // the preparation wave (nothing called: no private segment)
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) scalar_prep_one<true>(i, dig, rsig, ssig, nullptr, flags, prep_s[lane]);
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  const fer_consts k = fer_setup(lane);
  bool ok = false;
  const uint4* kt = ktab;
  row_comb_iso iso = {0u, 0u};
  if (sig < n) {
    const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)kidx[sig]);
    ok = key < nkeys && tinfo[key < nkeys ? key : 0u] != 0;
    if (ok) {                                                   // (wave-uniform)
      kt = ktab + (size_t)key * (KC_SLOTS * 8);
      iso = row_comb_iso_of(kt, k);
    }
  }
  __syncthreads();
  if (sig >= n) return;
  const uint32_t* p = prep_s[wave];
  if (!(ok && (p[16] & PF_OK))) {
    if (lane == 0) out[sig] = 0;
    return;
  }
  const pt29r acc = row_ladder_comb(kt, iso.w, iso.w3, p, false, gt, k);
  // ---- verdict: R != infinity and x(R) mod n == r (ecdsa.go:450-465), x(R) = X / Z ----
  uint8_t verdict = 0;
  if (!fer_is_zero(acc.z, k)) {
    uint32_t rw[8];
    load_be32(rw, rsig + (size_t)sig * 32);
    bool match = fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(fer_from_words(rw, k), acc.z, k), 1, k)), k);
    if (u256_lt(rw, FE_P_MINUS_N)) {
      uint32_t r2[8];
      u256_add(r2, rw, SC_N);
      match = match || fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(fer_from_words(r2, k), acc.z, k), 1, k)), k);
    }
    verdict = match ? 1 : 0;
  }
  if (lane == 0) out[sig] = verdict;
}

// FOUR LANES per signature (pt29q.h: a point is X | Y | Z | Z on the lanes of a quad, a layer of the complete formulas one lane
// product): the ladders for calls between the wave-per-signature kernels and the lane-per-signature ones - a
// doubling is 550 dependent instructions where a lane needs 1 070, so a lone wave is through its 16 signatures in half the
// time, at twice the instructions per signature.  Behind the preparation kernels (one lane per signature).
// quad_double_mult: u G + k1 Q + k2 lambda(Q) for the quad's signature, Q = (qx, qy) affine and on the curve; u | k1 | k2 | flags
// from the preparation's planes.  The key's table - (2j + 1) Q, j < 8, projective - lives in LDS, tab[entry][limb][lane]: the
// lanes of a quad hold x | y | z | beta * x of the entry (lane 3's copy of z is not read by an addition; lambda's image reads its
// x from there).  Returns this lane's coordinate of the result.
S2K_DEV fe29 quad_double_mult(const fe29& qx, const fe29& qy, uint32_t (*tab)[9][64], const uint32_t* __restrict__ prep, size_t stride,
                              uint32_t sig, uint32_t pf, gt_view gt, uint32_t lane) {
  const uint32_t q = lane & 3u;
  const fe29 beta = fe29_from_words(FE_BETA), one = fe29_one();
  {
    fe29 cur = fe29_pick(q >= 2, fe29_pick(q == 1, qx, qy), one);                  // x | y | 1 | 1
    const fe29 D = pt29q_double(cur, q);
#pragma unroll 1
    for (int j = 0; j < 8; ++j) {
      if (j) cur = pt29q_add(cur, D, q);
      const fe29 bx = fe29_mul(fe29_qperm<S2K_QP(0, 0, 0, 0)>(cur), beta);
      const fe29 st = fe29_pick(q == 3, cur, bx);
#pragma unroll
      for (int i = 0; i < 9; ++i) tab[j][i][lane] = st.n[i];
    }
  }
  // |k1|, |k2| odd, < 2^129
  sc k1 = sc_zero(), k2 = sc_zero();
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    k1.v[w] = prep[(size_t)(8 + w) * stride + sig];
    k2.v[w] = prep[(size_t)(12 + w) * stride + sig];
  }
  k1.v[4] = (pf & PF_K1_B128) ? 1u : 0u;
  k2.v[4] = (pf & PF_K2_B128) ? 1u : 0u;
  const bool neg1 = pf & PF_NEG1, neg2 = pf & PF_NEG2;
  digit_stream d1 = ds_init(k1), d2 = ds_init(k2);
  const uint32_t col3 = lane | 3u;
  auto entry_of = [&](uint32_t w, bool lam, bool sneg) -> fe29 {   // this lane's coordinate of the entry of digit w (2w - 15)
    const bool neg = sneg != (w < 8u);
    const uint32_t e = (w < 8u) ? (7u - w) : (w - 8u);
    const uint32_t col = (lam && q == 0) ? col3 : lane;            // lambda's image: x from the quad's fourth slot
    fe29 a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.n[i] = tab[e][i][col];
    return fe29_normalize_weak(fe29_cond_negate1(a, neg && q == 1));
  };
  fe29 acc = pt29q_add(entry_of(8u, false, neg1), entry_of(8u, true, neg2), q);     // the top digits are +1 (w = 8)
#pragma unroll 1
  for (int i = 31; i >= 0; --i) {
    const uint32_t w1 = ds_next(d1), w2 = ds_next(d2);
#pragma unroll 1
    for (int j = 0; j < 4; ++j) acc = pt29q_double(acc, q);
    acc = pt29q_add(acc, entry_of(w1, false, neg1), q);
    acc = pt29q_add(acc, entry_of(w2, true, neg2), q);
  }
  uint32_t u[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) u[w] = prep[(size_t)w * stride + sig];
  apt g = gt_load(gt, 0, gt_next_digit(u, gt.bits));
#pragma unroll 1
  for (uint32_t w = 0; w < gt.windows; ++w) {
    const fe29 qc = fe29_pick(q >= 2, fe29_pick(q == 1, fe29_from_words(g.x.v), fe29_from_words(g.y.v)), one);
    if (w + 1 < gt.windows) g = gt_load(gt, w + 1, gt_next_digit(u, gt.bits));
    acc = pt29q_add(acc, qc, q);
  }
  return acc;
}

// PublicKey.Verify (secec/ecdsa.go:171, 392-470), four lanes per signature; behind k_scalar_prep
__global__ void __launch_bounds__(256)
k_verify_quad(uint32_t n, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ rsig, const uint32_t* __restrict__ prep,
              gt_view gt, uint8_t* __restrict__ out, size_t stride) {
  __shared__ uint32_t tab_all[4][8][9][64];
  const uint32_t lane = threadIdx.x & 63u, q = lane & 3u;
  const uint32_t sig0 = (blockIdx.x * 256 + threadIdx.x) >> 2;
  const bool live = sig0 < n;
  const uint32_t sig = live ? sig0 : n - 1;                     // (idle quads redo the last signature: no divergence, no store)
  const uint32_t pf = prep[(size_t)16 * stride + sig];
  uint32_t xw[8], yw[8];
  load_be32(xw, pub + (size_t)sig * 64);
  load_be32(yw, pub + (size_t)sig * 64 + 32);
  bool ok = (pf & PF_OK) && fe_is_canonical_raw(xw) && fe_is_canonical_raw(yw);
  fe29 qx = fe29_from_words(xw), qy = fe29_from_words(yw);
  {   // y^2 == x^3 + 7 (point_s11n.go:298-307); an invalid key is replaced by G, its verdict is 0
    fe29 rhs = fe29_mul(fe29_sqr(qx), qx);
    rhs.n[0] += 7;
    if (!fe29_eq(fe29_sqr(qy), rhs)) ok = false;
    if (!ok) {
      qx = fe29_from_words(FE_GX);
      qy = fe29_from_words(FE_GY);
    }
  }
  const fe29 acc = quad_double_mult(qx, qy, tab_all[threadIdx.x >> 6], prep, stride, sig, pf, gt, lane);
  // ---- verdict: R != infinity and x(R) mod n == r (ecdsa.go:450-465), x(R) = X / Z ----
  const pt29 R = pt29q_gather(acc);
  uint8_t verdict = 0;
  if (ok && !fe29_is_zero(R.z)) {
    uint32_t rw[8];
    load_be32(rw, rsig + (size_t)sig * 32);
    bool match = fe29_eq(R.x, fe29_mul(fe29_from_words(rw), R.z));
    if (u256_lt(rw, FE_P_MINUS_N)) {
      uint32_t r2[8];
      u256_add(r2, rw, SC_N);
      match = match || fe29_eq(R.x, fe29_mul(fe29_from_words(r2), R.z));
    }
    verdict = match ? 1 : 0;
  }
  if (live && q == 0) out[sig] = verdict;
}

// SchnorrPublicKey.Verify (schnorr.go:221-253), four lanes per signature; behind k_schnorr_prep.  The two lifts - of the key and of
// r, the point R would have to be - run side by side on the lanes of the quad (lanes 0, 2: the key; lanes 1, 3: r), one chain of
// lane products; valid iff s G - e P is finite and equals (r, even y), compared projectively.
__global__ void __launch_bounds__(256)
k_schnorr_quad(uint32_t n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig64, const uint32_t* __restrict__ prep,
               gt_view gt, uint8_t* __restrict__ out, size_t stride) {
  __shared__ uint32_t tab_all[4][8][9][64];
  const uint32_t lane = threadIdx.x & 63u, q = lane & 3u;
  const uint32_t sig0 = (blockIdx.x * 256 + threadIdx.x) >> 2;
  const bool live = sig0 < n;
  const uint32_t sig = live ? sig0 : n - 1;
  const uint32_t pf = prep[(size_t)16 * stride + sig];
  uint32_t xw[8], rw[8];
  load_be32(xw, pk + (size_t)sig * 32);
  load_be32(rw, sig64 + (size_t)sig * 64);
  bool ok = (pf & PF_OK) && fe_is_canonical_raw(xw);            // (PF_OK: r < p, s < n)
  fe29 xP = fe29_from_words(xw);
  const fe29 xR = fe29_from_words(rw);
  const fe29 xin = fe29_pick((q & 1u) != 0, xP, xR);
  fe29 c = fe29_mul(fe29_sqr(xin), xin);
  c.n[0] += 7;
  fe29 y;
  const bool has = fe29_sqrt(y, c);
  y = fe29_normalize(y);
  y = fe29_pick((y.n[0] & 1u) != 0, y, fe29_normalize_weak(fe29_negate(y, 1)));       // the even root
  const int hasP = __builtin_amdgcn_mov_dpp(has ? 1 : 0, S2K_QP(0, 0, 0, 0), 0xF, 0xF, true);
  const int hasR = __builtin_amdgcn_mov_dpp(has ? 1 : 0, S2K_QP(1, 1, 1, 1), 0xF, 0xF, true);
  ok = ok && hasP && hasR;
  fe29 yP = fe29_qperm<S2K_QP(0, 0, 0, 0)>(y);
  const fe29 yR = fe29_qperm<S2K_QP(1, 1, 1, 1)>(y);
  if (!ok) {                                                    // keep the arithmetic on the curve; the verdict is 0
    xP = fe29_from_words(FE_GX);
    yP = fe29_from_words(FE_GY);
  }
  const fe29 acc = quad_double_mult(xP, yP, tab_all[threadIdx.x >> 6], prep, stride, sig, pf, gt, lane);
  const pt29 R = pt29q_gather(acc);
  uint8_t verdict = 0;
  if (ok && !fe29_is_zero(R.z))
    verdict = (fe29_eq(R.x, fe29_mul(xR, R.z)) && fe29_eq(R.y, fe29_mul(yR, R.z))) ? 1 : 0;
  if (live && q == 0) out[sig] = verdict;
}

// RecoverPublicKey (ecdsa.go:244-282), four lanes per item; between k_scalar_prep (u1 = -e/r, u2 = s/r, the id in the flags) and
// k_affine_finish<MODE_RECOVER>, which gets the Jacobian triple (X Z, Y Z^2, Z) it expects.  Items without a key: ok = 0 (their
// record was zeroed before).
__global__ void __launch_bounds__(256)
k_recover_quad(uint32_t n, const uint8_t* __restrict__ rsig, const uint32_t* __restrict__ prep, gt_view gt, uint32_t* __restrict__ fin,
               uint8_t* __restrict__ out, size_t stride) {
  __shared__ uint32_t tab_all[4][8][9][64];
  const uint32_t lane = threadIdx.x & 63u, q = lane & 3u;
  const uint32_t sig0 = (blockIdx.x * 256 + threadIdx.x) >> 2;
  const bool live = sig0 < n;
  const uint32_t sig = live ? sig0 : n - 1;
  const uint32_t pf = prep[(size_t)16 * stride + sig];
  const uint32_t rid = (pf >> 8) & 3u;
  uint32_t xw[8];
  load_be32(xw, rsig + (size_t)sig * 32);
  bool ok = (pf & PF_OK) != 0;                                  // (r, s in range, id < 4, r + n < p where the id asks for it)
  if (ok && (rid & 2u)) u256_add(xw, xw, SC_N);
  fe29 qx = fe29_from_words(xw);
  fe29 c = fe29_mul(fe29_sqr(qx), qx);
  c.n[0] += 7;
  fe29 qy;
  ok = fe29_sqrt(qy, c) && ok;
  qy = fe29_normalize(qy);
  qy = fe29_pick(((qy.n[0] & 1u) != 0) != ((rid & 1u) != 0), qy, fe29_normalize_weak(fe29_negate(qy, 1)));
  if (!ok) {
    qx = fe29_from_words(FE_GX);
    qy = fe29_from_words(FE_GY);
  }
  const fe29 acc = quad_double_mult(qx, qy, tab_all[threadIdx.x >> 6], prep, stride, sig, pf, gt, lane);
  const pt29 R = pt29q_gather(acc);
  const bool finite = !fe29_is_zero(R.z);                       // identity: NewPublicKeyFromPoint fails (secec.go:206-209)
  if (live && q == 0) {
    if (ok && finite) {
      const fe29 zz = fe29_sqr(R.z);
      fq_store(fin, stride, sig, 0, fe29_mul(R.x, R.z));
      fq_store(fin, stride, sig, 1, fe29_mul(R.y, zz));
      fq_store(fin, stride, sig, 2, R.z);
      out[sig] = VERDICT_PENDING;
    } else {
      out[sig] = 0;
    }
  }
}

// SchnorrPublicKey.Verify (schnorr.go:221-253) with one WAVEFRONT per signature (small batches; the block's fifth
// wave hashes the challenges and splits -e meanwhile).  lift_x of the key and of r - the point R would have to be - run as
// ONE chain of row products (rows 0, 1: the key; rows 2, 3: r): the signature is valid iff s G - e P is the point (r, even
// y), compared projectively, so there is no inversion.
// FUSED: five waves as described; the hashing makes that instance a 248-register kernel (two waves per SIMD), enough for up
// to 1024 signatures (1280 waves).  !FUSED (larger calls): four waves behind k_schnorr_prep, whose planes they read - 62 registers.
template <bool FUSED>
__global__ void __launch_bounds__(FUSED ? 320 : 256)
k_schnorr_row(uint32_t n, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ sig64, const uint8_t* __restrict__ msgs,
              const uint64_t* __restrict__ offs, uint32_t msg_len, const uint32_t* __restrict__ prep, size_t stride, gt_view gt,
              uint8_t* __restrict__ out) {
  __shared__ uint32_t tab_all[4][4][8][64];
  __shared__ uint32_t prep_s[4][20];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if constexpr (!FUSED) {
    const uint32_t i = blockIdx.x * 4 + wave;
    if (lane < 17 && i < n) prep_s[wave][lane] = prep[(size_t)lane * stride + i];
  }
  if (FUSED && wave == 4) {                                     // the preparation wave (k_schnorr_prep for four signatures)
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) {
      sc s, e;
      const bool ok = schnorr_parse(i, pk, sig64, msgs, offs, msg_len, s, e);     // (r < p, s < n)
      sc k1, k2;
      bool neg1, neg2;
      sc_split_glv_odd(sc_neg(e), k1, neg1, k2, neg2);          // schnorr.go:244
      uint32_t* o = prep_s[lane];
#pragma unroll
      for (int w = 0; w < 8; ++w) o[w] = s.v[w];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[8 + w] = k1.v[w];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[12 + w] = k2.v[w];
      o[16] = (ok ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) | (k1.v[4] ? PF_K1_B128 : 0) | (k2.v[4] ? PF_K2_B128 : 0);
    }
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  const fer_consts k = fer_setup(lane);
  bool ok = sig < n;
  fer xR = 0, yR = 0;
  if (ok) {
    uint32_t xw[8], rw[8];
    load_be32(xw, pk + (size_t)sig * 32);
    load_be32(rw, sig64 + (size_t)sig * 64);
    ok = fe_is_canonical_raw(xw);
    const fer xP = fer_from_words(xw, k);
    xR = fer_from_words(rw, k);
    const fer c = fer_curve_rhs(fer_sel2(k, xP, xR), k);
    const fer y = fer_sqrt_chain(c, k);
    const bool is_root = fer_is_zero(fer_add(fer_mul(y, y, k), fer_negate(c, 1, k)), k);     // (row by row)
    const bool odd = fer_is_odd(y, k);
    const fer y_even = fer_norm(odd ? fer_negate(y, 1, k) : y, k);
    const uint64_t roots = __builtin_amdgcn_ballot_w64(is_root);
    ok = ok && (roots & 1u) && ((roots >> 32) & 1u);            // both lifts exist (lane 0: the key, lane 32: r)
    pt29r Q1;
    Q1.x = xP;
    fer_halves(y_even, Q1.y, yR);
    Q1.z = k.j == 0 ? 1u : 0u;
    if (ok) row_table(Q1, tab_all[wave], k, lane);              // (wave-uniform)
  }
  __syncthreads();
  if (sig >= n) return;
  const uint32_t* p = prep_s[wave];
  if (!(ok && (p[16] & PF_OK))) {
    if (lane == 0) out[sig] = 0;
    return;
  }
  const pt29r acc = row_ladder(tab_all[wave], p, gt, k, lane);
  // R = s G - e P is finite, x(R) = r and y(R) is even: X = r Z and Y = y_r Z with Z != 0
  uint8_t verdict = 0;
  if (!fer_is_zero(acc.z, k)) {
    const bool mx = fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(xR, acc.z, k), 1, k)), k);
    const bool my = fer_is_zero(fer_add(fer_norm(acc.y, k), fer_negate(fer_mul(yR, acc.z, k), 1, k)), k);
    verdict = (mx && my) ? 1 : 0;
  }
  if (lane == 0) out[sig] = verdict;
}

// k_schnorr_row over a key set (row_ladder_keyset above).  The key needs no lift - the set holds X || Y, an odd stored Y flips
// both half scalars' signs as in k_verify_fast's key-set modes - but r does: one square-root chain per signature, about as
// long as the ladder itself.  It runs BESIDE the ladder: the block's sixth wave lifts the four r of the block in its four
// rows while the signature waves run; they read y_r (even) from LDS for the verdict only, behind a second barrier.  The
// fifth wave hashes the four challenges (over the set's X) and splits -e, as in k_schnorr_row<true>.
__global__ void __launch_bounds__(384)
k_schnorr_row_keyset(uint32_t n, uint32_t nkeys, const uint32_t* __restrict__ kidx, const uint8_t* __restrict__ set_keys,
                     const uint4* __restrict__ ktab, const uint8_t* __restrict__ tinfo, const uint8_t* __restrict__ sig64,
                     const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len, gt_view gt,
                     uint8_t* __restrict__ out) {
  __shared__ uint32_t prep_s[4][20];
  __shared__ uint32_t yr_s[4][16];          // y_r of the block's signatures, limb j at word j; word 15: r is an x of the curve
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wave == 4) {                                              // the preparation wave
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) {
      const uint32_t key = kidx[i];
      sc s, e;
      const bool ok = schnorr_parse_key(i, set_keys + (size_t)(key < nkeys ? key : 0u) * 64, sig64, msgs, offs, msg_len, s, e);   // (r < p, s < n)
      sc k1, k2;
      bool neg1, neg2;
      sc_split_glv_odd(sc_neg(e), k1, neg1, k2, neg2);          // schnorr.go:244
      uint32_t* o = prep_s[lane];
#pragma unroll
      for (int w = 0; w < 8; ++w) o[w] = s.v[w];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[8 + w] = k1.v[w];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[12 + w] = k2.v[w];
      o[16] = (ok ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) | (k1.v[4] ? PF_K1_B128 : 0) | (k2.v[4] ? PF_K2_B128 : 0);
    }
    __syncthreads();
    __syncthreads();
    return;
  }
  const fer_consts k = fer_setup(lane);
  if (wave == 5) {                                              // the lifting wave: row i takes r of the block's signature i
    __syncthreads();
    const uint32_t i = blockIdx.x * 4 + k.row;
    uint32_t rw[8];
    load_be32(rw, sig64 + (size_t)(i < n ? i : n - 1) * 64);
    const fer c = fer_curve_rhs(fer_from_words(rw, k), k);
    const fer y = fer_sqrt_chain(c, k);
    const bool is_root = fer_is_zero(fer_add(fer_mul(y, y, k), fer_negate(c, 1, k)), k);     // (row by row)
    const fer y_even = fer_norm(fer_is_odd(y, k) ? fer_negate(y, 1, k) : y, k);
    yr_s[k.row][k.j] = k.j == 15 ? (is_root ? 1u : 0u) : y_even;
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  bool ok = false, flip = false;
  const uint4* kt = ktab;
  row_iso iso = {0u, 0u, 0u};
  if (sig < n) {
    const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)kidx[sig]);
    ok = key < nkeys && tinfo[key < nkeys ? key : 0u] != 0;
    if (ok) {                                                   // (wave-uniform)
      kt = ktab + (size_t)key * (KS_SLOTS * 8);
      iso = row_iso_of(kt, k);
      flip = (set_keys[(size_t)key * 64 + 63] & 1u) != 0;       // BIP-340 multiplies lift_x(X): the point with even Y
    }
  }
  __syncthreads();
  const uint32_t* p = prep_s[wave];
  ok = ok && (p[16] & PF_OK);
  pt29r acc = pt29r_identity(k);
  if (ok) acc = row_ladder_keyset(kt, iso, p, flip, gt, k);     // (wave-uniform)
  __syncthreads();
  if (sig >= n) return;
  // R = s G - e P is finite, x(R) = r and y(R) is even: X = r Z and Y = y_r Z with Z != 0
  uint8_t verdict = 0;
  if (ok && yr_s[wave][15] && !fer_is_zero(acc.z, k)) {
    uint32_t rw[8];
    load_be32(rw, sig64 + (size_t)sig * 64);
    const fer xR = fer_from_words(rw, k), yR = k.j <= 8 ? yr_s[wave][k.j] : 0u;
    const bool mx = fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(xR, acc.z, k), 1, k)), k);
    const bool my = fer_is_zero(fer_add(fer_norm(acc.y, k), fer_negate(fer_mul(yR, acc.z, k), 1, k)), k);
    verdict = (mx && my) ? 1 : 0;
  }
  if (lane == 0) out[sig] = verdict;
}

// k_schnorr_row_keyset over a comb set (row_ladder_comb): the same six waves and the same two barriers
__global__ void __launch_bounds__(384)
k_schnorr_row_comb(uint32_t n, uint32_t nkeys, const uint32_t* __restrict__ kidx, const uint8_t* __restrict__ set_keys,
                   const uint4* __restrict__ ktab, const uint8_t* __restrict__ tinfo, const uint8_t* __restrict__ sig64,
                   const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len, gt_view gt,
                   uint8_t* __restrict__ out) {
  __shared__ uint32_t prep_s[4][20];
  __shared__ uint32_t yr_s[4][16];          // y_r of the block's signatures, limb j at word j; word 15: r is an x of the curve
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wave == 4) {                                              // the preparation wave (nothing called: no private segment)
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) {
      const uint32_t key = kidx[i];
      sc s, e;
      const bool ok = schnorr_parse_key<true>(i, set_keys + (size_t)(key < nkeys ? key : 0u) * 64, sig64, msgs, offs, msg_len, s, e);   // (r < p, s < n)
      sc k1, k2;
      bool neg1, neg2;
      sc_split_glv_odd(sc_neg(e), k1, neg1, k2, neg2);          // schnorr.go:244
      uint32_t* o = prep_s[lane];
#pragma unroll
      for (int w = 0; w < 8; ++w) o[w] = s.v[w];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[8 + w] = k1.v[w];
#pragma unroll
      for (int w = 0; w < 4; ++w) o[12 + w] = k2.v[w];
      o[16] = (ok ? PF_OK : 0) | (neg1 ? PF_NEG1 : 0) | (neg2 ? PF_NEG2 : 0) | (k1.v[4] ? PF_K1_B128 : 0) | (k2.v[4] ? PF_K2_B128 : 0);
    }
    __syncthreads();
    __syncthreads();
    return;
  }
  const fer_consts k = fer_setup(lane);
  if (wave == 5) {                                              // the lifting wave: row i takes r of the block's signature i
    __syncthreads();
    const uint32_t i = blockIdx.x * 4 + k.row;
    uint32_t rw[8];
    load_be32(rw, sig64 + (size_t)(i < n ? i : n - 1) * 64);
    const fer c = fer_curve_rhs(fer_from_words(rw, k), k);
    const fer y = fer_sqrt_chain(c, k);
    const bool is_root = fer_is_zero(fer_add(fer_mul(y, y, k), fer_negate(c, 1, k)), k);     // (row by row)
    const fer y_even = fer_norm(fer_is_odd(y, k) ? fer_negate(y, 1, k) : y, k);
    yr_s[k.row][k.j] = k.j == 15 ? (is_root ? 1u : 0u) : y_even;
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  bool ok = false, flip = false;
  const uint4* kt = ktab;
  row_comb_iso iso = {0u, 0u};
  if (sig < n) {
    const uint32_t key = (uint32_t)__builtin_amdgcn_readfirstlane((int)kidx[sig]);
    ok = key < nkeys && tinfo[key < nkeys ? key : 0u] != 0;
    if (ok) {                                                   // (wave-uniform)
      kt = ktab + (size_t)key * (KC_SLOTS * 8);
      iso = row_comb_iso_of(kt, k);
      flip = (set_keys[(size_t)key * 64 + 63] & 1u) != 0;       // BIP-340 multiplies lift_x(X): the point with even Y
    }
  }
  __syncthreads();
  const uint32_t* p = prep_s[wave];
  ok = ok && (p[16] & PF_OK);
  pt29r acc = pt29r_identity(k);
  if (ok) acc = row_ladder_comb(kt, iso.w, iso.w3, p, flip, gt, k);     // (wave-uniform)
  __syncthreads();
  if (sig >= n) return;
  // R = s G - e P is finite, x(R) = r and y(R) is even: X = r Z and Y = y_r Z with Z != 0
  uint8_t verdict = 0;
  if (ok && yr_s[wave][15] && !fer_is_zero(acc.z, k)) {
    uint32_t rw[8];
    load_be32(rw, sig64 + (size_t)sig * 64);
    const fer xR = fer_from_words(rw, k), yR = k.j <= 8 ? yr_s[wave][k.j] : 0u;
    const bool mx = fer_is_zero(fer_add(acc.x, fer_negate(fer_mul(xR, acc.z, k), 1, k)), k);
    const bool my = fer_is_zero(fer_add(fer_norm(acc.y, k), fer_negate(fer_mul(yR, acc.z, k), 1, k)), k);
    verdict = (mx && my) ? 1 : 0;
  }
  if (lane == 0) out[sig] = verdict;
}

// RecoverPublicKey (ecdsa.go:244-282) with one WAVEFRONT per item (small batches; the block's fifth wave computes
// u1 = -e/r, u2 = s/r meanwhile): R = (r or r + n, the root of the asked parity) by a chain of row products, Q = u1 G + u2 R
// on the complete formulas, 1/Z by the inversion chain in row products, the 65-byte record written by the wave.  Items
// without a key get ok = 0 and the zero record.
__global__ void __launch_bounds__(320)
k_recover_row(uint32_t n, const uint8_t* __restrict__ dig, const uint8_t* __restrict__ rsig, const uint8_t* __restrict__ ssig,
              const uint8_t* __restrict__ recid, gt_view gt, uint8_t* __restrict__ out, uint8_t* __restrict__ out_pts) {
  __shared__ uint32_t tab_all[4][4][8][64];
  __shared__ uint32_t prep_s[4][20];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  if (wave == 4) {                                              // the preparation wave
    const uint32_t i = blockIdx.x * 4 + lane;
    if (lane < 4 && i < n) scalar_prep_one(i, dig, rsig, ssig, recid, 0u, prep_s[lane]);
    __syncthreads();
    return;
  }
  const uint32_t sig = blockIdx.x * 4 + wave;
  const fer_consts k = fer_setup(lane);
  bool ok = sig < n;
  if (ok) {
    const uint32_t rid = recid[sig];
    uint32_t xw[8];
    load_be32(xw, rsig + (size_t)sig * 32);
    if (rid & 2u) u256_add(xw, xw, SC_N);                       // (that r + n < p holds is the preparation wave's check)
    pt29r Q1;
    Q1.x = fer_from_words(xw, k);
    Q1.z = k.j == 0 ? 1u : 0u;
    const fer c = fer_curve_rhs(Q1.x, k);
    const fer y = fer_sqrt_chain(c, k);
    ok = fer_is_zero(fer_add(fer_mul(y, y, k), fer_negate(c, 1, k)), k);
    Q1.y = fer_norm(fer_is_odd(y, k) != ((rid & 1u) != 0) ? fer_negate(y, 1, k) : y, k);
    if (ok) row_table(Q1, tab_all[wave], k, lane);              // (wave-uniform)
  }
  __syncthreads();
  if (sig >= n) return;
  uint8_t* rec = out_pts + (size_t)sig * 65;
  auto no_key = [&]() {                                         // ok = 0 and the zero record (RecoverPublicKey's error)
    rec[lane] = 0;
    if (lane == 0) {
      rec[64] = 0;
      out[sig] = 0;
    }
  };
  const uint32_t* p = prep_s[wave];
  if (!(ok && (p[16] & PF_OK))) {                               // (r, s in range, id < 4, r + n < p where the id asks for it)
    no_key();
    return;
  }
  const pt29r acc = row_ladder(tab_all[wave], p, gt, k, lane);
  if (fer_is_zero(acc.z, k)) {                                  // identity: NewPublicKeyFromPoint fails (secec.go:206-209)
    no_key();
    return;
  }
  const fer zi = fer_inv_chain(acc.z, k);
  uint32_t xw[8], yw[8];
  fe29_to_words(xw, fe29_normalize(fer_to_fe29(fer_mul(acc.x, zi, k))));
  fe29_to_words(yw, fe29_normalize(fer_to_fe29(fer_mul(fer_norm(acc.y, k), zi, k))));
  if (lane == 0) {
    rec[0] = 0x04;
    store_be32_unaligned(rec + 1, xw);
    store_be32_unaligned(rec + 33, yw);
    out[sig] = 1;
  }
}

// The launchers (engine_internal.h; the rule they follow: lane_kernels.hip).  launch_schnorr_row is the only place that names an
// instantiation of k_schnorr_row: prep == nullptr is k_schnorr_row<true>, whose fifth wave prepares.
__attribute__((visibility("hidden"))) void launch_verify_row(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                              uint32_t flags, uint8_t* out) {
  k_verify_row<<<(unsigned)((n + 3) / 4), 320, 0, st>>>((uint32_t)n, pub, dig, r, s, flags, ctx->gt_call, out);
}
__attribute__((visibility("hidden"))) void launch_verify_row_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint4* ktab,
                                     const uint8_t* tinfo, const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_verify_row_keyset<<<(unsigned)((n + 3) / 4), 320, 0, st>>>((uint32_t)n, (uint32_t)nkeys, kidx, ktab, tinfo, dig, r, s, flags, ctx->gt_call,
                                                               out);
}
__attribute__((visibility("hidden"))) void launch_verify_row_comb(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint4* ktab,
                                   const uint8_t* tinfo, const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out) {
  k_verify_row_comb<<<(unsigned)((n + 3) / 4), 320, 0, st>>>((uint32_t)n, (uint32_t)nkeys, kidx, ktab, tinfo, dig, r, s, flags, ctx->gt_call, out);
}
__attribute__((visibility("hidden"))) void launch_schnorr_row(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs,
                               const uint64_t* offs, uint32_t msg_len, const uint32_t* prep, size_t stride, uint8_t* out) {
  if (!prep)
    k_schnorr_row<true><<<(unsigned)((n + 3) / 4), 320, 0, st>>>((uint32_t)n, pk, sig, msgs, offs, msg_len, nullptr, 0, ctx->gt_call, out);
  else
    k_schnorr_row<false><<<(unsigned)((n + 3) / 4), 256, 0, st>>>((uint32_t)n, pk, sig, msgs, offs, msg_len, prep, stride, ctx->gt_call, out);
}
__attribute__((visibility("hidden"))) void launch_schnorr_row_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint8_t* set_keys,
                                      const uint4* ktab, const uint8_t* tinfo, const uint8_t* sig, const uint8_t* msgs, const uint64_t* offs,
                                      uint32_t msg_len, uint8_t* out) {
  k_schnorr_row_keyset<<<(unsigned)((n + 3) / 4), 384, 0, st>>>((uint32_t)n, (uint32_t)nkeys, kidx, set_keys, ktab, tinfo, sig, msgs, offs,
                                                                msg_len, ctx->gt_call, out);
}
__attribute__((visibility("hidden"))) void launch_schnorr_row_comb(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint8_t* set_keys,
                                    const uint4* ktab, const uint8_t* tinfo, const uint8_t* sig, const uint8_t* msgs, const uint64_t* offs,
                                    uint32_t msg_len, uint8_t* out) {
  k_schnorr_row_comb<<<(unsigned)((n + 3) / 4), 384, 0, st>>>((uint32_t)n, (uint32_t)nkeys, kidx, set_keys, ktab, tinfo, sig, msgs, offs,
                                                              msg_len, ctx->gt_call, out);
}
__attribute__((visibility("hidden"))) void launch_recover_row(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                               const uint8_t* recid, uint8_t* ok, uint8_t* pub65) {
  k_recover_row<<<(unsigned)((n + 3) / 4), 320, 0, st>>>((uint32_t)n, dig, r, s, recid, ctx->gt_call, ok, pub65);
}
__attribute__((visibility("hidden"))) void launch_verify_quad(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pub, const uint8_t* r, const lane_ws& w, uint8_t* out) {
  k_verify_quad<<<(unsigned)((n + 63) / 64), 256, 0, st>>>((uint32_t)n, pub, r, w.prep, ctx->gt_call, out, w.stride);
}
__attribute__((visibility("hidden"))) void launch_schnorr_quad(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* sig, const lane_ws& w, uint8_t* out) {
  k_schnorr_quad<<<(unsigned)((n + 63) / 64), 256, 0, st>>>((uint32_t)n, pk, sig, w.prep, ctx->gt_call, out, w.stride);
}
__attribute__((visibility("hidden"))) void launch_recover_quad(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* r, const lane_ws& w, uint8_t* out) {
  k_recover_quad<<<(unsigned)((n + 63) / 64), 256, 0, st>>>((uint32_t)n, r, w.prep, ctx->gt_call, w.fin, out, w.stride);
}
