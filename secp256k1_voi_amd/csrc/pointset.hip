// pointset.hip — point sets: segmented multi-scalar multiplication over a FIXED list of points whose tables are kept across calls,
//   out[j] = sum_{i in [off[j], off[j+1])} k_i * P[point_index[i]]      (Point.MultiScalarMultVartime per segment on the expanded slice)
//
// msm_seg.hip builds a table {1 .. 8} * P per term (one inversion each) and runs 128 doublings per piece in EVERY call, even when
// every sum of every call runs over the same points.  A point set (s2k_pointset_*, the sibling of s2k_keyset) does that work
// once: for every point and every digit position pos of a C-bit signed recoding of a 128-bit half scalar it keeps
//   entry (pos, mag) = mag * 2^(C pos) * P      1 <= mag <= 2^(C-1),    true affine, 64 bytes of canonical words (msm_seg_shared.h)
// so that a term is 2 * POS table additions (both half scalars of the endomorphism split; the lambda half multiplies x by
// beta as k_seg_ladder does) and NO doubling: 66 additions at C = 4 (POS = 33), 34 at C = 8 (POS = 17).  The last position only
// ever holds the recoding's carry digit (0 or 1); the layout is uniform all the same (every position has 2^(C-1) entries).
//
// Table layout: [position][point][magnitude].  The ladder walks the positions in its OUTER loop (there are no doublings, so the
// order of the additions is free), which makes the device as a whole sweep the tables slab by slab: one position of a 64-point
// set is 512 KiB at C = 8, where the whole set (8.5 MiB) is larger than an XCD's L2.
//
//   build          k_ps_chain      one lane per point: the record judged by msm_classify_record29 (msm_terms.h), the chain
//                                  B_pos = 2^(C pos) * P by Jacobian doublings, made affine with one inversion per point
//                                  (prefix products of the Z) and stored as entry (pos, 1).
//                  k_ps_multiples  one lane per (point, position): 2 B by a Jacobian doubling, 3 B .. 2^(C-1) B by Jacobian mixed
//                                  additions of B (jacobian29.h), one inversion per lane: Z_(j+1) = Z_j * H_j, so 1 / Z_top and
//                                  the H (parked in scratch) give every 1 / Z_j on the way back.
//                  These chains hold the ONLY incomplete formulas of the file.  A doubling of a point of prime order is never
//                  exceptional; the additions' operands are j * B and B for 2 <= j < 2^(C-1) <= 128 with B of prime order n:
//                  never equal, never opposite, never the identity.  Lanes of identity records store nothing; the digits of
//                  terms that name such a point are forced to zero by the front kernel.
//   call           host plan       the plan of msm_seg.hip (s2k_internal_seg_plan_build) with this call's piece length and crossover.
//                  k_ps_front      one lane per term: the point index resolved (dense shape: the term's position in its segment)
//                                  and checked, the scalar reduced as SetBytes, split with sc_split_glv, both magnitudes recoded
//                                  into POS signed C-bit digits by adding the constant with bit C-1 of every digit set (no carry
//                                  chain; the top position takes the carry).  One 16-BIT WORD per digit in position-major planes:
//                                  the magnitude (0 .. 2^(C-1): 128 needs bit 7 itself at C = 8) in bits 0-8, bit 15 set when the
//                                  addend is to be negated (digit sign times half-scalar sign); a zero digit is the word 0.
//                  k_ps_ladder     one lane per piece: per position the signed-digit additions of the piece's 2 * len half
//                                  scalars, pt29_add_mixed at the lazy-field codes of k_seg_ladder (the affine addend at one unit,
//                                  -y brought back to one unit); the entry of the next addition is fetched while this one runs,
//                                  the digit and the point index of the one after that beside it.
//                  k_seg_combine   (msm_seg_shared.h) the pieces of a segment summed, one inversion, the 65-byte record.
//                  long segments   (more than `crossover` terms) k_ps_gather expands the set's stored records into the workspace
//                                  and the bucket method of msm.hip takes them, exactly as msm_seg.hip hands its long segments on.
//
// The ladder's and the combine step's additions are complete (pt29.h): P + P (a point twice in a set or a segment), P - P and an
// identity accumulator are simply right, there is no flag and no second path.
#include <cstdlib>

#include <vector>

#include "msm_internal.h"
#include "msm_terms.h"
#include "fe29_inv.h"
#include "jacobian29.h"
#include "pt29.h"
#include "sc.h"
#include "msm_seg_shared.h"

#ifndef S2K_POINTSET_T
#define S2K_POINTSET_T 8               // terms per piece (one ladder lane); S2K_POINTSET_T in the environment overrides it (1 .. 64)
#endif
#ifndef S2K_POINTSET_CROSSOVER
#define S2K_POINTSET_CROSSOVER 16384   // segments longer than this take the bucket method; S2K_POINTSET_CROSSOVER overrides it
#endif
#ifndef S2K_POINTSET_WAVES
#define S2K_POINTSET_WAVES 3           // waves per SIMD the ladder kernel is built for (at most 168 VGPRs)
#endif

struct s2k_pointset {
  s2k_ctx* ctx;          // the owner (compared, never followed after creation)
  uint64_t generation;   // of the owner: a context destroyed and another created at the same address is not the owner
  int device;
  size_t m;
  int c;                 // digit width: 4 or 8
  uint8_t* base;         // device: tables | records (m * 65) | flags (m) | status word
  size_t bytes, o_rec, o_flag, o_status;
};

namespace {

constexpr size_t PS_ENTRY_BYTES = 64, PS_PT_WORDS = 27;    // a table entry (msm_seg_shared.h); a piece sum: x, y, z of 9 limbs

template <int C>
struct ps_geom {
  static_assert(C == 4 || C == 8, "digit widths of a point set");
  static constexpr uint32_t POS = 128 / C + 1;             // digit positions of a recoded 128-bit magnitude (the last: the carry)
  static constexpr uint32_t E = 1u << (C - 1);             // entries per position: 1 .. 2^(C-1) times the position's base
  static constexpr uint32_t ADDC = C == 4 ? 0x88888888u : 0x80808080u;   // bit C-1 of every digit
  static constexpr size_t POINT_BYTES = (size_t)POS * E * PS_ENTRY_BYTES;
};
constexpr uint32_t PS_FINITE = TERM_FINITE, PS_MALFORMED = TERM_MALFORMED;   // per-point flag (0: the identity record): msm_terms.h
constexpr uint32_t PS_ST_RECORD = 1, PS_ST_INDEX = 2;       // status word of a call
constexpr uint32_t PS_NEG = 0x8000u, PS_MAG = 0x1ffu;       // digit word

size_t ps_point_bytes(int c) { return c == 4 ? ps_geom<4>::POINT_BYTES : ps_geom<8>::POINT_BYTES; }
size_t ps_scratch_bytes(size_t m, int c) { return m * ps_point_bytes(c) / 2; }     // 32 bytes per entry (k_ps_multiples: the H)

uint32_t ps_default_T() {
  const char* e = getenv("S2K_POINTSET_T");
  const int t = e ? atoi(e) : S2K_POINTSET_T;
  return (uint32_t)(t < 1 ? 1 : (t > (int)SEG_T_MAX ? (int)SEG_T_MAX : t));
}
uint64_t ps_default_crossover() {
  const char* e = getenv("S2K_POINTSET_CROSSOVER");
  const long long c = e ? atoll(e) : (long long)S2K_POINTSET_CROSSOVER;
  return (uint64_t)(c < 1 ? 1 : c);
}

// nullptr: the arguments are fine
const char* ps_check(size_t m, size_t n, bool indexed, size_t n_seg, const uint64_t* off) {
  if (const char* e = seg_check(n, n_seg, off)) return e;
  if (!indexed)
    for (size_t j = 0; j < n_seg; ++j)
      if (off[j + 1] - off[j] > (uint64_t)m) return "dense segment longer than the point set";
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// build
// ---------------------------------------------------------------------------------------------------------------------
S2K_DEV size_t ps_entry_quad(uint32_t m, uint32_t E, uint32_t pos, uint32_t i, uint32_t mag) {   // 1 <= mag <= E
  return (((size_t)pos * m + i) * E + (mag - 1u)) * 4;
}
S2K_DEV void ps_store_fe(uint4* __restrict__ e, const fe29& a) {
  uint32_t w[8];
  fe29_to_words(w, fe29_normalize(a));
  e[0] = make_uint4(w[0], w[1], w[2], w[3]);
  e[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
S2K_DEV fe29 ps_load_fe(const uint4* __restrict__ e) {
  const uint4 a = e[0], b = e[1];
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  return fe29_from_words(w);
}
// the entry at e holds Jacobian X, Y of a point whose 1 / Z is zi: make it affine in place
S2K_DEV void ps_entry_affine(uint4* __restrict__ e, const fe29& zi) {
  fe29 X, Y;
  seg_entry_point(seg_entry_fetch(e), X, Y);
  const fe29 zi2 = fe29_sqr(zi), zi3 = fe29_mul(zi2, zi);
  seg_entry_store(e, fe29_mul(X, zi2), fe29_mul(Y, zi3));
}

// One lane per point: record check, flags, and entry (pos, 1) = 2^(C pos) * P for every position.
// scratch: 64 bytes per (point, position): Z_pos and the prefix product Z_0 ... Z_pos.
template <int C>
__global__ void __launch_bounds__(256)
k_ps_chain(uint32_t m, const uint8_t* __restrict__ recs, uint8_t* __restrict__ flags, uint4* __restrict__ tbl, uint4* __restrict__ scratch,
           uint32_t* __restrict__ status) {
  using G = ps_geom<C>;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const uint8_t* rec = recs + (size_t)i * 65;
  fe29 px, py;
  const uint32_t f = msm_classify_record29(rec, px, py);
  flags[i] = (uint8_t)f;
  if (f == PS_MALFORMED) atomicOr(status, PS_ST_RECORD);
  if (f != PS_FINITE) return;                           // (an identity record has no table: its terms' digits are zero)
  uint4* scr = scratch + (size_t)i * G::POS * 4;
  jpt29 cur;
  cur.x = px;
  cur.y = py;
  cur.z = fe29_one();
  fe29 pre = fe29_one();
#pragma unroll 1
  for (uint32_t pos = 0; pos < G::POS; ++pos) {
    seg_entry_store(tbl + ps_entry_quad(m, G::E, pos, i, 1), cur.x, cur.y);   // (parked as they are; made affine below)
    pre = fe29_mul(pre, cur.z);
    seg_entry_store(scr + (size_t)pos * 4, cur.z, pre);
    if (pos + 1 < G::POS) {
#pragma unroll 1
      for (int t = 0; t < C; ++t) cur = jpt29_double(cur);
    }
  }
  fe29 inv = fe29_inv_gcd(fe29_normalize_weak(pre));    // 1 / (Z_0 ... Z_top)
#pragma unroll 1
  for (uint32_t pos = G::POS - 1; pos >= 1; --pos) {    // (position 0 is the point itself: Z = 1)
    const fe29 z = ps_load_fe(scr + (size_t)pos * 4);                  // Z_pos
    const fe29 before = ps_load_fe(scr + (size_t)(pos - 1) * 4 + 2);   // Z_0 ... Z_(pos-1)
    ps_entry_affine(tbl + ps_entry_quad(m, G::E, pos, i, 1), fe29_mul(inv, before));
    inv = fe29_mul(inv, z);
  }
}

// One lane per (point, position): entries 2 .. E from entry 1 (B, affine).  scratch: 32 bytes per entry: H of the addition that
// made it.  The additions' operands are j * B and B, 2 <= j < E <= 128, B of prime order: never equal, opposite or the identity.
template <int C>
__global__ void __launch_bounds__(256)
k_ps_multiples(uint32_t m, const uint8_t* __restrict__ flags, uint4* __restrict__ tbl, uint4* __restrict__ scratch) {
  using G = ps_geom<C>;
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= (size_t)m * G::POS) return;
  const uint32_t pos = (uint32_t)(id / m), i = (uint32_t)(id % m);
  if (flags[i] != PS_FINITE) return;
  uint4* e = tbl + ps_entry_quad(m, G::E, pos, i, 1);
  uint4* hs = scratch + (((size_t)pos * m + i) * G::E) * 2;
  fe29 bx, by;
  seg_entry_point(seg_entry_fetch(e), bx, by);
  jpt29 cur;
  cur.x = bx;
  cur.y = by;
  cur.z = fe29_one();
  cur = jpt29_double(cur);
  seg_entry_store(e + 4, cur.x, cur.y);                 // (parked as they are; made affine below)
#pragma unroll 1
  for (uint32_t mag = 3; mag <= G::E; ++mag) {
    fe29 h;
    cur = jpt29_add_affine(cur, bx, by, &h);
    seg_entry_store(e + (size_t)(mag - 1) * 4, cur.x, cur.y);
    ps_store_fe(hs + (size_t)(mag - 1) * 2, h);
  }
  fe29 zi = fe29_inv_gcd(fe29_normalize_weak(cur.z));   // 1 / Z_E
#pragma unroll 1
  for (uint32_t mag = G::E; mag >= 2; --mag) {          // zi = 1 / Z_mag
    ps_entry_affine(e + (size_t)(mag - 1) * 4, zi);
    if (mag >= 3) zi = fe29_mul(zi, ps_load_fe(hs + (size_t)(mag - 1) * 2));   // 1 / Z_(mag-1) = H_mag / Z_mag
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// call
// ---------------------------------------------------------------------------------------------------------------------
// A magnitude k < 2^128 as POS signed digits: k + ADDC has the C-bit digits d_p + 2^(C-1) with d_p in -2^(C-1) .. 2^(C-1) - 1 and
// k = sum_p d_p 2^(C p); the last digit is the carry out of bit 128 (0 or 1).  (tests/pointset_model.py is the big-integer model.)
template <int C>
S2K_DEV void ps_store_digits(uint16_t* __restrict__ dg, size_t plane, size_t at, const sc& k, bool neg, bool zero) {
  using G = ps_geom<C>;
  uint32_t w[5];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c += (uint64_t)k.v[i] + G::ADDC;
    w[i] = (uint32_t)c;
    c >>= 32;
  }
  w[4] = (uint32_t)c;
#pragma unroll 1
  for (uint32_t pos = 0; pos < G::POS; ++pos) {
    const uint32_t bit = pos * C;
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) word = (bit >> 5) == (uint32_t)i ? w[i] : word;
    const int v = (int)((word >> (bit & 31u)) & ((1u << C) - 1u));
    const int d = pos + 1 < G::POS ? v - (int)G::E : v;
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    const bool flip = (d < 0) != neg;
    dg[(size_t)pos * plane + at] = (zero || mag == 0) ? (uint16_t)0 : (uint16_t)(mag | (flip ? PS_NEG : 0u));
  }
}

// pieces: [first term among the Straus terms | length | destination | first term of the input | source] x npieces, `source` the
// position in its segment of the piece's first term (dense shape) or its position in the input (indexed shape).
template <int C>
__global__ void __launch_bounds__(256)
k_ps_front(uint32_t npieces, uint32_t T, uint32_t NS, const uint32_t* __restrict__ pieces, const uint8_t* __restrict__ scalars,
           const uint32_t* __restrict__ point_index, uint32_t m, const uint8_t* __restrict__ flags, uint16_t* __restrict__ dg,
           uint32_t* __restrict__ tix, uint32_t* __restrict__ status) {
  const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t p = (uint32_t)(id / T), j = (uint32_t)(id % T);
  if (p >= npieces || j >= pieces[(size_t)npieces + p]) return;
  const size_t c = (size_t)pieces[p] + j, i = (size_t)pieces[3 * (size_t)npieces + p] + j;
  uint32_t idx = point_index ? point_index[i] : pieces[4 * (size_t)npieces + p] + j;
  bool zero = false;
  if (idx >= m) {                                       // names no point: S2K_ERR_ARG for the call
    atomicOr(status, PS_ST_INDEX);
    idx = 0;
    zero = true;
  }
  zero = zero || flags[idx] != PS_FINITE;               // an identity record contributes nothing
  tix[c] = idx;
  uint32_t raw[8];
  load_be32(raw, scalars + i * 32);
  const sc k = sc_reduce_once(raw);                     // SetBytes semantics (scalar.go:123)
  sc k1, k2;
  bool neg1, neg2;
  sc_split_glv(k, k1, neg1, k2, neg2);
  const size_t plane = 2 * (size_t)NS;
  ps_store_digits<C>(dg, plane, 2 * c, k1, neg1, zero);
  ps_store_digits<C>(dg, plane, 2 * c + 1, k2, neg2, zero);
}

// (a zero digit asks for the point's first entry: a valid address, never used; for an identity record it was never written)
S2K_DEV const uint4* ps_entry_addr(const uint4* __restrict__ slab, uint32_t E, uint32_t idx, uint32_t word) {
  const uint32_t mag = word & PS_MAG;
  return slab + ((size_t)idx * E + (mag ? mag - 1u : 0u)) * 4;
}

template <int C>
__global__ void __launch_bounds__(256, S2K_POINTSET_WAVES)
k_ps_ladder(uint32_t npieces, uint32_t NS, uint32_t m, const uint32_t* __restrict__ pieces, const uint16_t* __restrict__ dg,
            const uint32_t* __restrict__ tix, const uint4* __restrict__ tbl, uint32_t* __restrict__ sums, size_t stride) {
  using G = ps_geom<C>;
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npieces) return;
  const uint32_t first = pieces[p] /* among the Straus terms */, len = pieces[npieces + p], steps = 2u * len, dest = pieces[2 * (size_t)npieces + p];
  const size_t plane = 2 * (size_t)NS;
  const uint32_t* __restrict__ ix = tix + first;
  const fe29 beta = seg_beta();
  pt29 acc = pt29_identity();
#pragma unroll 1
  for (uint32_t pos = 0; pos < G::POS; ++pos) {
    const uint16_t* __restrict__ d = dg + (size_t)pos * plane + 2 * (size_t)first;
    const uint4* __restrict__ slab = tbl + (size_t)pos * m * (G::E * 4);     // this position's entries of every point
    uint32_t b_cur = d[0], b_nxt = d[1];                                     // (steps >= 2: a piece has at least one term)
    uint32_t i_nxt = ix[0];                                                  // step 1 is the first term's lambda half
    seg_raw r_cur = seg_entry_fetch(ps_entry_addr(slab, G::E, i_nxt, b_cur));
#pragma unroll 1
    for (uint32_t s = 0; s < steps; ++s) {
      fe29 qx, qy;
      seg_entry_point(r_cur, qx, qy);
      // the next entry (past the end: the last term's first entry, a valid address) and the digit and index after it
      const seg_raw r_nxt = seg_entry_fetch(ps_entry_addr(slab, G::E, i_nxt, b_nxt));
      const uint32_t b_nn = s + 2 < steps ? d[s + 2] : 0u;
      const uint32_t t_nn = (s + 2) >> 1;
      const uint32_t i_nn = ix[t_nn < len ? t_nn : len - 1u];
      if (b_cur & PS_MAG) {
        if (s & 1u) qx = fe29_mul(qx, beta);                                 // the lambda half: (beta x, y)
        if (b_cur & PS_NEG) qy = fe29_normalize_weak(fe29_negate(qy, 1));    // -y at one unit
        acc = pt29_add_mixed(acc, qx, qy);
      }
      r_cur = r_nxt;
      b_cur = b_nxt;
      b_nxt = b_nn;
      i_nxt = i_nn;
    }
  }
#pragma unroll
  for (int w = 0; w < 9; ++w) {
    sums[(size_t)w * stride + dest] = acc.x.n[w];
    sums[(size_t)(9 + w) * stride + dest] = acc.y.n[w];
    sums[(size_t)(18 + w) * stride + dest] = acc.z.n[w];
  }
}

// terms [a, a + L) of a long segment: their points' records, for the bucket method
__global__ void __launch_bounds__(256)
k_ps_gather(uint32_t a, uint32_t L, const uint32_t* __restrict__ point_index, uint32_t m, const uint8_t* __restrict__ recs,
            uint8_t* __restrict__ out, uint32_t* __restrict__ status) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= L) return;
  const uint32_t idx = point_index ? point_index[(size_t)a + t] : t;
  uint8_t* o = out + (size_t)t * 65;
  if (idx >= m) {
    atomicOr(status, PS_ST_INDEX);
    for (int b = 0; b < 65; ++b) o[b] = 0;
    return;
  }
  const uint8_t* r = recs + (size_t)idx * 65;
  for (int b = 0; b < 65; ++b) o[b] = r[b];
}

struct ps_carve {
  size_t o_status, o_segdesc, o_pieces, o_tix, o_digits, o_sums, o_gather, bytes;
};
ps_carve ps_workspace(const seg_plan& p, size_t n_seg, uint32_t positions, size_t long_terms) {
  ps_carve w;
  size_t o = 0;
  auto carve = [&](size_t bytes) { size_t at = o; o = seg_align(o + bytes, 256); return at; };
  w.o_status = carve(256);
  w.o_segdesc = carve(n_seg * 8);
  w.o_pieces = carve(p.n_pieces * 20);
  w.o_tix = carve(p.n_short_terms * 4);
  w.o_digits = carve(p.n_short_terms * 2 * positions * 2);
  w.o_sums = carve(p.piece_stride * PS_PT_WORDS * 4);
  w.o_gather = carve(long_terms * 65);
  w.bytes = o;
  return w;
}

template <int C>
void ps_launch(hipStream_t st, const seg_plan& p, uint32_t m, const uint32_t* d_pieces, const uint8_t* sc_in, const uint32_t* d_index,
               const uint8_t* flags, uint16_t* d_digits, uint32_t* d_tix, const uint4* tbl, uint32_t* d_sums, uint32_t* d_status) {
  const size_t np = p.n_pieces;
  k_ps_front<C><<<blocks_for(np * p.T), 256, 0, st>>>((uint32_t)np, p.T, (uint32_t)p.n_short_terms, d_pieces, sc_in, d_index, m, flags, d_digits,
                                                        d_tix, d_status);
  k_ps_ladder<C><<<blocks_for(np), 256, 0, st>>>((uint32_t)np, (uint32_t)p.n_short_terms, m, d_pieces, d_digits, d_tix, tbl, d_sums, p.piece_stride);
}

template <int C>
void ps_build(hipStream_t st, const s2k_pointset* ps, uint4* scratch) {
  const uint32_t m = (uint32_t)ps->m;
  uint4* tbl = (uint4*)ps->base;
  uint8_t* flags = ps->base + ps->o_flag;
  k_ps_chain<C><<<blocks_for(m), 256, 0, st>>>(m, ps->base + ps->o_rec, flags, tbl, scratch, (uint32_t*)(ps->base + ps->o_status));
  k_ps_multiples<C><<<blocks_for((size_t)m * ps_geom<C>::POS), 256, 0, st>>>(m, flags, tbl, scratch);
}

bool ps_owned(const s2k_ctx* ctx, const s2k_pointset* ps) {
  const s2k_ctx* owner = ctx->parent ? ctx->parent : ctx;
  return ps && ps->ctx == owner && ps->generation == owner->generation && ps->device == ctx->device;
}

}  // namespace

extern "C" {

int s2k_pointset_geometry(int window_bits, uint64_t out[3]) {
  if (!out || (window_bits != 4 && window_bits != 8)) return fail(nullptr, S2K_ERR_ARG, "point-set digit width is 4 or 8");
  out[0] = window_bits == 4 ? ps_geom<4>::POS : ps_geom<8>::POS;
  out[1] = window_bits == 4 ? ps_geom<4>::E : ps_geom<8>::E;
  out[2] = ps_point_bytes(window_bits);
  return S2K_OK;
}

int s2k_pointset_create(s2k_ctx* ctx, size_t m, const uint8_t* points65, int window_bits, s2k_pointset** out) {
  if (!ctx || !out) return fail(ctx, S2K_ERR_ARG, "null argument");
  *out = nullptr;
  if (window_bits != 0 && window_bits != 4 && window_bits != 8) return fail(ctx, S2K_ERR_ARG, "point-set digit width is 0 (automatic), 4 or 8");
  if (m == 0 || !points65) return fail(ctx, S2K_ERR_ARG, "empty point set");
  if (m > 0x0fffffffu) return fail(ctx, S2K_ERR_ARG, "point set too large");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  // what counts as free: the device's free memory less what the background generator-table build is about to take, capped by
  // the keyset_free_bytes budget.  Automatic: 8 bits when the tables take at most half of that, else 4 bits by the same rule.
  // An explicit width has to fit the budget (when one is set) and the device.
  const size_t budget = s2k_internal_keyset_budget();
  int c = window_bits;
  if (c == 0) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
    const size_t promised = s2k_internal_gt_pending_bytes(ctx->device);
    free_b -= promised < free_b ? promised : free_b;
    if (budget && free_b > budget) free_b = budget;
    if (m * ps_point_bytes(8) <= free_b / 2) c = 8;
    else if (m * ps_point_bytes(4) <= free_b / 2) c = 4;
    else return fail(ctx, S2K_ERR_NOMEM, "point set of %zu points: %zu bytes at 4-bit digits do not fit half of the %zu bytes free", m, m * ps_point_bytes(4), free_b);
  } else if (budget && m * ps_point_bytes(c) > budget) {
    return fail(ctx, S2K_ERR_NOMEM, "point set of %zu points at %d-bit digits: %zu bytes exceed the table budget", m, c, m * ps_point_bytes(c));
  }
  s2k_pointset* ps = new (std::nothrow) s2k_pointset();
  if (!ps) return fail(ctx, S2K_ERR_NOMEM, "out of host memory");
  ps->ctx = ctx;
  ps->generation = ctx->generation;
  ps->device = ctx->device;
  ps->m = m;
  ps->base = nullptr;
  uint4* scratch = nullptr;
  for (;;) {                                            // (an automatic 8 whose allocation fails all the same falls to 4 once)
    ps->c = c;
    ps->o_rec = seg_align(m * ps_point_bytes(c), 256);
    ps->o_flag = ps->o_rec + seg_align(m * 65, 256);
    ps->o_status = ps->o_flag + seg_align(m, 256);
    ps->bytes = ps->o_status + 256;
    hipError_t e = hipMalloc((void**)&ps->base, ps->bytes);
    if (e == hipSuccess) {
      e = hipMalloc((void**)&scratch, ps_scratch_bytes(m, c));
      if (e != hipSuccess) {
        (void)hipFree(ps->base);
        ps->base = nullptr;
      }
    }
    if (e == hipSuccess) break;
    (void)hipGetLastError();
    if (window_bits == 0 && c == 8) {
      c = 4;
      continue;
    }
    delete ps;
    return fail(ctx, S2K_ERR_NOMEM, "point set of %zu points at %d-bit digits: %s", m, c, hipGetErrorString(e));
  }
  hipStream_t st = ctx->s_comp;
  uint32_t h_status = 0;
  rc = ctx_enter(ctx, st);
  if (rc == S2K_OK && (hipMemcpyAsync(ps->base + ps->o_rec, points65, m * 65, hipMemcpyHostToDevice, st) != hipSuccess ||
                       hipMemsetAsync(ps->base + ps->o_status, 0, 256, st) != hipSuccess))
    rc = fail(ctx, S2K_ERR_HIP, "copy of the point records failed");
  if (rc == S2K_OK) {
    if (c == 4) ps_build<4>(st, ps, scratch);
    else ps_build<8>(st, ps, scratch);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_status, ps->base + ps->o_status, 4, hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = fail(ctx, S2K_ERR_HIP, "point set build failed to launch");
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == S2K_OK) rc = fail(ctx, S2K_ERR_HIP, "point set build failed");
  (void)hipFree(scratch);
  ctx->have_last = false;
  if (rc == S2K_OK && h_status) rc = fail(ctx, S2K_ERR_ARG, "malformed point record in the point set");
  if (rc) {
    (void)hipFree(ps->base);
    delete ps;
    return rc;
  }
  *out = ps;
  return S2K_OK;
}

void s2k_pointset_destroy(s2k_pointset* ps) {
  if (!ps) return;
  (void)hipSetDevice(ps->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(ps->base);
  delete ps;
}
size_t s2k_pointset_size(const s2k_pointset* ps) { return ps ? ps->m : 0; }
int s2k_pointset_window_bits(const s2k_pointset* ps) { return ps ? ps->c : 0; }
size_t s2k_pointset_device_bytes(const s2k_pointset* ps) { return ps ? ps->bytes : 0; }

int s2k_debug_pointset_entry(const s2k_pointset* ps, size_t i, unsigned pos, unsigned mag, uint8_t out64[64]) {
  if (!ps || !out64) return fail(nullptr, S2K_ERR_ARG, "null argument");
  uint64_t g[3];
  (void)s2k_pointset_geometry(ps->c, g);
  if (i >= ps->m || pos >= g[0] || mag < 1 || mag > g[1]) return fail(nullptr, S2K_ERR_ARG, "no such table entry");
  HIP_TRY(nullptr, hipSetDevice(ps->device));
  uint8_t flag = 0;
  HIP_TRY(nullptr, hipMemcpy(&flag, ps->base + ps->o_flag + i, 1, hipMemcpyDeviceToHost));
  memset(out64, 0, 64);
  if (flag != PS_FINITE) return S2K_OK;                 // the identity record: no table
  uint32_t w[16];
  const size_t quad = (((size_t)pos * ps->m + i) * g[1] + (mag - 1)) * 4;
  HIP_TRY(nullptr, hipMemcpy(w, ps->base + quad * 16, 64, hipMemcpyDeviceToHost));
  for (int half = 0; half < 2; ++half)
    for (int j = 0; j < 8; ++j) {
      const uint32_t v = w[half * 8 + (7 - j)];
      uint8_t* q = out64 + half * 32 + j * 4;
      q[0] = (uint8_t)(v >> 24); q[1] = (uint8_t)(v >> 16); q[2] = (uint8_t)(v >> 8); q[3] = (uint8_t)v;
    }
  return S2K_OK;
}

int s2k_debug_pointset_check_args(size_t m, size_t n, int indexed, size_t n_seg, const uint64_t* seg_offsets) {
  if (const char* e = ps_check(m, n, indexed != 0, n_seg, seg_offsets)) return fail(nullptr, S2K_ERR_ARG, "%s", e);
  return S2K_OK;
}

int s2k_pointset_multi_scalar_mult_segments_device(s2k_ctx* ctx, const s2k_pointset* ps, size_t n, const void* d_k, const void* d_point_index,
                                                   size_t n_seg, const uint64_t* seg_offsets, void* d_out, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!ps_owned(ctx, ps)) return fail(ctx, S2K_ERR_ARG, "point set of another context");
  if (n_seg && !d_out) return fail(ctx, S2K_ERR_ARG, "null output buffer");
  if (n && !d_k) return fail(ctx, S2K_ERR_ARG, "null input buffer");
  if (const char* e = ps_check(ps->m, n, d_point_index != nullptr, n_seg, seg_offsets)) return fail(ctx, S2K_ERR_ARG, "%s", e);
  if (n_seg == 0) return S2K_OK;
  seg_plan p;
  if (const char* e = s2k_internal_seg_plan_build(n, n_seg, seg_offsets, ps_default_T(), ps_default_crossover(), p)) return fail(ctx, S2K_ERR_ARG, "%s", e);
  size_t long_terms = 0;
  for (size_t j : p.longs) long_terms += (size_t)(seg_offsets[j + 1] - seg_offsets[j]);
  const uint32_t positions = ps->c == 4 ? ps_geom<4>::POS : ps_geom<8>::POS;
  const ps_carve w = ps_workspace(p, n_seg, positions, long_terms);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  // both workspaces are brought to their final size before the first launch (growing one frees it)
  rc = ctx_reserve(ctx, &ctx->seg_ws, &ctx->seg_ws_bytes, w.bytes);
  if (rc) return rc;
  for (size_t j : p.longs) {
    rc = s2k_internal_msm_reserve(ctx, (size_t)(seg_offsets[j + 1] - seg_offsets[j]));
    if (rc) return rc;
  }
  uint8_t* ws = (uint8_t*)ctx->seg_ws;
  uint32_t* d_status = (uint32_t*)(ws + w.o_status);
  uint32_t* d_segdesc = (uint32_t*)(ws + w.o_segdesc);
  uint32_t* d_pieces = (uint32_t*)(ws + w.o_pieces);
  uint32_t* d_sums = (uint32_t*)(ws + w.o_sums);
  const uint8_t* sc_in = (const uint8_t*)d_k;
  const uint32_t* d_index = (const uint32_t*)d_point_index;
  const uint8_t* recs = ps->base + ps->o_rec;
  uint8_t* out = (uint8_t*)d_out;
  HIP_TRY(ctx, hipMemsetAsync(d_status, 0, 256, st));
  if (p.n_long < n_seg) {
    // the plan goes up in ONE copy from the context's pinned block, as in msm_seg.hip: segment descriptors and, behind them as in
    // the workspace, the five piece arrays
    const size_t np = p.n_pieces, bytes = (w.o_pieces - w.o_segdesc) + np * 20;
    if (bytes > ctx->seg_host_bytes) {
      if (ctx->seg_host) HIP_TRY(ctx, hipHostFree(ctx->seg_host));
      ctx->seg_host = nullptr;
      ctx->seg_host_bytes = 0;
      HIP_TRY(ctx, hipHostMalloc(&ctx->seg_host, bytes, hipHostMallocDefault));
      ctx->seg_host_bytes = bytes;
    }
    uint8_t* h = (uint8_t*)ctx->seg_host;
    memcpy(h, p.segdesc.data(), n_seg * 8);
    uint32_t* hp = (uint32_t*)(h + (w.o_pieces - w.o_segdesc));
    if (np) {
      memcpy(hp, p.cfirst.data(), np * 4);
      memcpy(hp + np, p.len.data(), np * 4);
      memcpy(hp + 2 * np, p.dest.data(), np * 4);
      memcpy(hp + 3 * np, p.first.data(), np * 4);
      if (d_index) {
        memcpy(hp + 4 * np, p.first.data(), np * 4);      // (unused: the index array names the point)
      } else {
        // dense shape: piece number `id` in segment order starts at position t of its segment
        std::vector<uint32_t> tpos(np);
        size_t id = 0;
        for (size_t j = 0; j < n_seg; ++j) {
          const size_t L = (size_t)(seg_offsets[j + 1] - seg_offsets[j]);
          if ((uint64_t)L > p.crossover) continue;
          for (size_t t = 0; t < L; t += p.T) tpos[id++] = (uint32_t)t;
        }
        for (size_t at = 0; at < np; ++at) hp[4 * np + at] = tpos[p.dest[at]];
      }
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_segdesc, h, bytes, hipMemcpyHostToDevice, st));
  }
  if (p.n_pieces) {
    if (ps->c == 4)
      ps_launch<4>(st, p, (uint32_t)ps->m, d_pieces, sc_in, d_index, ps->base + ps->o_flag, (uint16_t*)(ws + w.o_digits), (uint32_t*)(ws + w.o_tix),
                   (const uint4*)ps->base, d_sums, d_status);
    else
      ps_launch<8>(st, p, (uint32_t)ps->m, d_pieces, sc_in, d_index, ps->base + ps->o_flag, (uint16_t*)(ws + w.o_digits), (uint32_t*)(ws + w.o_tix),
                   (const uint4*)ps->base, d_sums, d_status);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (p.n_long < n_seg) {
    k_seg_combine<<<blocks_for(n_seg), 256, 0, st>>>((uint32_t)n_seg, d_segdesc, d_sums, p.piece_stride, out);
    HIP_TRY(ctx, hipGetLastError());
  }
  size_t g_at = 0;
  for (size_t j : p.longs) {                            // the bucket method, one segment at a time, no synchronisation between them
    const size_t a = (size_t)seg_offsets[j], L = (size_t)(seg_offsets[j + 1] - seg_offsets[j]);
    uint8_t* d_pts = ws + w.o_gather + g_at * 65;
    g_at += L;
    k_ps_gather<<<blocks_for(L), 256, 0, st>>>((uint32_t)a, (uint32_t)L, d_index, (uint32_t)ps->m, recs, d_pts, d_status);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t* d_st = nullptr;
    rc = s2k_internal_msm_enqueue(ctx, st, L, sc_in + a * 32, d_pts, out + j * 65, &d_st);
    if (rc) return rc;
    k_seg_or_status<<<1, 1, 0, st>>>(d_st, d_status);
    HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t h_status = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&h_status, d_status, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;   // the stream has been synchronised: nothing of this context is in flight
  if (h_status & PS_ST_INDEX) return fail(ctx, S2K_ERR_ARG, "point index beyond the point set");
  if (h_status) return fail(ctx, S2K_ERR_ARG, "malformed point record in multi-scalar multiplication input");
  return S2K_OK;
}

int s2k_pointset_multi_scalar_mult_segments(s2k_ctx* ctx, const s2k_pointset* ps, size_t n, const uint8_t* k, const uint32_t* point_index,
                                            size_t n_seg, const uint64_t* seg_offsets, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (!ps_owned(ctx, ps)) return fail(ctx, S2K_ERR_ARG, "point set of another context");
  if (n_seg && !out) return fail(ctx, S2K_ERR_ARG, "null output buffer");
  if (n && !k) return fail(ctx, S2K_ERR_ARG, "null input buffer");
  if (const char* e = ps_check(ps->m, n, point_index != nullptr, n_seg, seg_offsets)) return fail(ctx, S2K_ERR_ARG, "%s", e);
  if (n_seg == 0) return S2K_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  const size_t sizes[3] = {n * 32 + 16, n * 4 + 16, n_seg * 65 + 16};
  uint8_t* d[3];
  rc = ctx_stage(ctx, sizes, 3, d);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  s2k_phase_guard phase(ctx->device, n * 36);
  if (n) {
    HIP_TRY(ctx, hipMemcpyAsync(d[0], k, n * 32, hipMemcpyHostToDevice, st));
    if (point_index) HIP_TRY(ctx, hipMemcpyAsync(d[1], point_index, n * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(ctx, phase.landed(st));
  rc = s2k_pointset_multi_scalar_mult_segments_device(ctx, ps, n, d[0], point_index ? d[1] : nullptr, n_seg, seg_offsets, d[2], st);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out, d[2], n_seg * 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return S2K_OK;
}

}  // extern "C"
