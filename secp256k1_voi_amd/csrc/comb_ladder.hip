// comb_ladder.hip — the comb ladders of the grouped ECDSA and BIP-340 calls and of comb key sets, in a kernel of their own:
// k_verify_comb<false> runs where k_verify_fast<MODE_ECDSA_COMB> ran, k_verify_comb<true> where <MODE_SCHNORR_COMB> did
// (lane_kernels.hip: launch_ladder; S2K_COMB_LEAD=1 brings those two back).  Same tables (kc_geom, keyed.hip), same arguments,
// same verdicts; what differs is how the ladder starts.
//
// The recoding.  An odd half scalar k < 2^129 over the comb's L = 133 digit positions (7 teeth, 19 bits apart):
//   k_verify_fast     k = 2^133 + sum_{i<133} (2 a_i - 1) 2^i,  a = k >> 1            the lead 2^133 Q goes in first, with Z = 1,
//                                                                                     and column 18 is a full addition to it
//   here              k =         sum_{i<133} (2 a'_i - 1) 2^i, a' = (k >> 1) | 2^132 since sum (2 a'_i - 1) 2^i = 2 a' - (2^133 - 1)
// a has 128 bits, so a' is a with bit 18 of the top tooth set and every other digit as it was: the top tooth is positive in
// column 18 (it was negative there, as it still is in columns 14..17) and that difference of 2 * 2^132 is the lead.  Column 18
// then STARTS the accumulator: the sum of its two entries, T = (t.x, -t.ny) over Z h, is a Jacobian point as it stands.  The
// lead lookup, jpt29_rescale (2 M), jpt29_add_affine (8 M + 3 S) and acc.z * h (1 M) of that column are not run: 14 of its 20
// products, 512 of the ladder's 526.  Nothing reads the table's LEAD slots from here; the table kernels still write them (the
// window ladders' tables share the layout, and k_verify_fast<.._COMB> reads them).
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "complete_path.h"
#include "jacobian29.h"
#include "lane_tables.h"
#include "sc.h"

using namespace s2k;

// MODE_ECDSA_COMB (SCHNORR = false) / MODE_SCHNORR_COMB (true) of k_verify_fast (verify_fast.h, where the arguments, the lane
// mapping and the verdict rules are described): lane idx of the launch's part handles signature kg.perm[idx] on the comb
// table kg.ptab[idx]; the generator part u1 G comes from kg.gp (k_generator_part).
template <bool SCHNORR>
__global__ void __launch_bounds__(256, S2K_COMB_WAVES)
k_verify_comb(uint32_t n_and_flags, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ rsig,
              const uint32_t* __restrict__ prep, uint32_t* __restrict__ qt, uint32_t* __restrict__ fin,
              gt_view gt, uint8_t* __restrict__ out, uint32_t* __restrict__ wl_count,
              uint32_t* __restrict__ wl, size_t stride, uint8_t* __restrict__ out_pts, uint64_t* __restrict__ clk,
              key_groups kg) {
  (void)qt;        // (the arguments of k_verify_fast, so that launch_ladder passes one list: no per-lane table, no resident
  (void)gt;        // generator table and no point records here)
  (void)out_pts;
  const bool force_wl = (n_and_flags & KVF_FORCE_WORKLIST) != 0;
  const uint32_t n = n_and_flags & ~KVF_FORCE_WORKLIST;
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;         // lane: workspace column
  uint32_t lo = 0, hi = kg.counters[KG_NKEYED];
  if (kg.nparts > 1) {                                         // two-part flow: this launch takes one side of the split
    const uint32_t sp = kg.counters[KG_SPLIT_LANE];
    if (kg.part) lo = sp;
    else hi = sp;
  }
  idx += lo;
  if (idx >= hi) return;
  const uint32_t lanes = hi - lo;
  const size_t sig = kg.perm[idx];                             // signature: input / prep / verdict column
  // effective shader clock of this launch (bench.py roofline), as k_verify_fast stamps it: wave 0 of the first and of the
  // last workgroup
  const bool stamp = clk != nullptr && (blockIdx.x == 0 || blockIdx.x == (lanes - 1) / 256) && threadIdx.x < 64;
  uint64_t t0c = 0, t0w = 0;
  if (stamp) {
    t0c = __builtin_readcyclecounter();
    t0w = __builtin_amdgcn_s_memrealtime();
  }
  const uint32_t pf = prep[(size_t)16 * stride + sig];
  const bool ok = (pf & PF_OK) && kg.tinfo[kg.ptab[idx]];      // the key was validated when its table was built
  bool neg1 = pf & PF_NEG1, neg2 = pf & PF_NEG2;
  if constexpr (SCHNORR) {
    // a comb key set holds X || Y (kg.key_bytes == 64; pub = the set's keys): BIP-340 multiplies the point with EVEN y, so an
    // odd Y changes both half scalars' signs.  The tables of a call are those of the lifted keys: nothing to do.  The test is
    // uniform over the launch
    if (kg.key_bytes == 64) {
      const bool y_odd = (pub[(size_t)kg.ptab[idx] * 64 + 63] & 1u) != 0;
      neg1 = neg1 != y_odd;
      neg2 = neg2 != y_odd;
    }
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
  using G = kc_geom;
  const uint4* kt = kg.ktab + (size_t)kg.ptab[idx] * (G::SLOTS * 8);
  // tooth t of a half: bits 19 t .. 19 t + 18 of a' (tooth 6: 14 bits of a = k >> 1, zeros, and bit 18 set); bit j of it is a
  // shift and a mask.  The 19 columns of both halves (7 + 7 bits) are cut once and wait in LDS, one word per round and lane
  // ([round][lane]: no two lanes of a wave share a bank, no lane reads another's): 19 KiB per block, and no register held
  // across the ladder.
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
    t1[G::TEETH - 1] |= 1u << (G::SPACING - 1);                                 // a' = a | 2^132: the lead, as a digit
    t2[G::TEETH - 1] |= 1u << (G::SPACING - 1);
#pragma unroll
    for (int j = 0; j < G::SPACING; ++j) {
      uint32_t w = 0;
#pragma unroll
      for (int t = 0; t < G::TEETH; ++t) w |= (((t1[t] >> j) & 1u) << t) | (((t2[t] >> j) & 1u) << (8 + t));
      cols[j][threadIdx.x] = w;
    }
  }
  jpt29 acc;
  {
    // round 18, peeled: the column's pair sum IS the accumulator.  E1 of the first half and phi(E2) of the second are affine
    // over the table's Z, their sum T = (t.x, -t.ny) stands over Z h: Jacobian coordinates with Z = h on the table's curve
    // (4 M + 2 S, where the loop's column spends 15 M + 5 S).  h = 0 (E1 = +-phi(E2)) leaves Z = 0 from the start: sticky, and
    // the lane ends on the worklist as from any other round.
    const uint32_t w12 = cols[G::SPACING - 1][threadIdx.x], w1 = w12 & 127u, w2 = w12 >> 8;
    const bool top1 = (w1 & 64u) != 0, top2 = (w2 & 64u) != 0;                 // (set above: both positive)
    const bool n1 = neg1 != !top1, n2 = neg2 != !top2;
    fe29 x1, y1, x2, y2;
    ke_load_xy(kt + (size_t)((top1 ? w1 : ~w1) & 63u) * 8, false, x1, y1);
    ke_load_xy(kt + (size_t)((top2 ? w2 : ~w2) & 63u) * 8, true, x2, y2);
    const coz29_sum t = coz29_pair_sum(x1, y1, x2, fe29_cond_negate1(y2, n1 != n2));   // x1 [1] y1 [1] x2 [1] y2 [<= 2]
    acc.x = t.x;                                       // [1]
    acc.y = fe29_cond_negate1(t.ny, !n1);              // [1] -> [<= 2]   (ny = -Y_T: negated unless E1 is negative)
    acc.z = t.h;                                       // [1]   weakly normalised
  }
  // rounds 17..0: the doubling, which takes x [1], y [<= 2], z [1] - the peeled round's point, or the column's - and the
  // column.  18 doublings and 18 columns, the loop's blocks all run 18 times.
#pragma unroll 1
  for (int j = G::SPACING - 2; j >= 0; --j) {
    acc = jpt29_double(acc);
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
  }
  // the table's points are affine on the curve isomorphic by W (keyed.hip): back on secp256k1 itself
  // (W is asked for here and not in front of the ladder: nothing is held across it but the accumulator)
  acc.z = fe29_mul(acc.z, ke_load(kt + (size_t)G::WENT * 8, G::W));

  // ---- generator part: u1*G, computed by k_generator_part ----
  // (final_only: Z was not 0 BEFORE the last addition and the addend is finite - then a zero after it arose in that addition,
  // and the verdict code below decides it instead of queueing the lane for the complete-formula kernel)
  bool final_only = false;
  {
    jpt29 q;
    q.x = fq_load(kg.gp, stride, sig, 0);
    q.y = fq_load(kg.gp, stride, sig, 1);
    q.z = fq_load(kg.gp, stride, sig, 2);
    if constexpr (!SCHNORR) final_only = !fe29_is_zero(acc.z) && !fe29_is_zero(q.z);
    acc = jpt29_add(acc, q);
  }

  // ---- verdict ---- (the rules of k_verify_fast, verify_fast.h: Z = 0 first seen in the final addition of two finite points
  // is decided here - X3 != 0: opposite points, R is the identity; X3 = 0: equal points, the worklist kernel doubles u1 G -,
  // every other zero goes to the worklist untagged)
  uint8_t verdict = 0;
  bool undecided = ok && fe29_is_zero(acc.z), is_identity = false;
  uint32_t wl_tag = 0;
  if constexpr (!SCHNORR) {
    if (force_wl && ok) {                                // S2K_ECDSA_FORCE_WORKLIST (diagnostic)
      undecided = true;
      final_only = false;
    }
    if (undecided && final_only) {
      if (!fe29_is_zero(acc.x)) {
        undecided = false;
        is_identity = true;                              // P - P
      } else if (n < WL_TAG_LIMIT) {
        wl_tag = WL_DOUBLE_GEN;                          // P + P: R = 2 u1 G
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
    } else if constexpr (SCHNORR) {
      // affine epilogue (even-y test) needs 1/Z: leave (X, Y, Z) in the SIGNATURE's fin column and let k_affine_finish
      // share one inversion between 16
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

// the two instantiations launch_ladder (lane_kernels.hip) launches
template __global__ void k_verify_comb<false>(uint32_t, const uint8_t*, const uint8_t*, const uint32_t*, uint32_t*, uint32_t*, gt_view, uint8_t*,
                                              uint32_t*, uint32_t*, size_t, uint8_t*, uint64_t*, key_groups);
template __global__ void k_verify_comb<true>(uint32_t, const uint8_t*, const uint8_t*, const uint32_t*, uint32_t*, uint32_t*, gt_view, uint8_t*,
                                             uint32_t*, uint32_t*, size_t, uint8_t*, uint64_t*, key_groups);
