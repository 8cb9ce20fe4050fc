// verify_fast.h — the lane-per-signature ladder kernel, k_verify_fast<MODE>, and what only it uses (digit_stream4).  The
// ladder_*.hip units include this file and instantiate their modes, each MODE_* in exactly one of them; launch_ladder
// (lane_kernels.hip) launches them through the declaration in engine_internal.h.
#pragma once
#include <hip/hip_runtime.h>

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
// (S2K_JOINT_WAVES itself, the comb ladders' bound, S2K_COMB_WAVES, and VERDICT_PENDING: engine_internal.h)

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
// (128 VGPRs, 96 spilled) 11.45 ms.  (S2K_FAST_WAVES: engine_internal.h)

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

// One line of a ladder_*.hip unit: the explicit instantiation of mode M (the unit list of launch_ladder, lane_kernels.hip)
#define S2K_LADDER_INSTANCE(M)                                                                                                     \
  template __global__ void k_verify_fast<M>(uint32_t, const uint8_t*, const uint8_t*, const uint32_t*, uint32_t*, uint32_t*, gt_view, \
                                            uint8_t*, uint32_t*, uint32_t*, size_t, uint8_t*, uint64_t*, key_groups);
