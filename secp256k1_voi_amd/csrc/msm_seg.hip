// msm_seg.hip — segmented multi-scalar multiplication on gfx950: many independent sums per call,
//   out[j] = sum_{i in [off[j], off[j+1])} k_i * P_i      (Point.MultiScalarMultVartime per segment, point_mul_multi.go:73-117)
//
// msm.hip computes ONE sum with the bucket method, whose sort / reduce / tail stages are latency bound and do not shrink
// with the input; a caller with thousands of short sums cannot pay them per sum.  Short segments therefore run Straus
// (the reference's own algorithm, :73-117) in pieces of T terms, the doublings shared inside a PIECE (a 64-term segment at
// T = 8 is 8 ladders of 128 doublings each, summed afterwards), all pieces of all segments side by side:
//
//   host plan      (seg_plan_build, a pure function: s2k_debug_msm_segments_plan exposes it to the tests) every segment of at
//                  most `crossover` terms is cut into PIECES of at most T consecutive terms; the pieces are ordered by length,
//                  longest first, so that the lanes of a wave run the same number of additions.  Longer segments go to msm.hip.
//   k_seg_front    one lane per term (of the short segments): scalar reduced as SetBytes, record judged by
//                  msm_classify_record29 (msm_terms.h), endomorphism split (two 128-bit magnitudes with signs), both recoded into 33 signed 4-bit
//                  digits (-8 .. 7, by adding 0x88..8: no carry chain), one byte per digit in position-major planes; and the
//                  table {1 .. 8} * P: a Jacobian chain (one doubling, six mixed additions: jacobian29.h, the chain k_key_odd
//                  runs), brought to TRUE affine with one safegcd inversion per term (the Z of entry j is the Z of entry
//                  j - 1 times the H of the addition, so 1 / Z_8 and the H give every 1 / Z_j).  Tables of different terms meet
//                  in one accumulator, so keyed.hip's common-Z curve trick does not carry over.  64 bytes per entry (canonical
//                  words), 512 bytes per term, in the workspace; the lambda half uses the same table with beta * x.
//   k_seg_ladder   one lane per piece: per digit position (32 .. 0) four doublings of ONE accumulator and the signed-digit
//                  additions of the piece's 2 * len half scalars, the table entry of the next addition fetched while this one
//                  runs and the digit of the one after that beside it.
//   k_seg_combine  one lane per short segment: its pieces summed (pt29_add), one inversion, the 65-byte record; an empty
//                  segment writes the identity record (:37).
//
// EVERY addition and doubling of the ladder and of the combine step is a complete formula (pt29.h: pt29_add_mixed, pt29_double,
// pt29_add, the lazy-field codes the bucket path's redo already runs): an accumulator that meets P + P, P - P or the identity in
// the middle of a ladder is simply right, there is no flag and no second path.  The only incomplete formulas are those of the
// table chain, whose operands are j * P and P for 2 <= j <= 7 with P of prime order n: never equal, opposite or the identity.
#include <cstdlib>

#include <vector>

#include "msm_internal.h"
#include "msm_terms.h"
#include "fe29_inv.h"
#include "jacobian29.h"
#include "pt29.h"
#include "sc.h"
#include "msm_seg_shared.h"

#ifndef S2K_MSM_SEG_T
#define S2K_MSM_SEG_T 8            // terms per piece (one ladder lane); S2K_MSM_SEG_T in the environment overrides it (1 .. 64)
#endif
#ifndef S2K_MSM_SEG_CROSSOVER
#define S2K_MSM_SEG_CROSSOVER 16384  // segments longer than this take the bucket method; S2K_MSM_SEG_CROSSOVER overrides it
#endif
#ifndef S2K_MSM_SEG_WAVES
#define S2K_MSM_SEG_WAVES 3        // waves per SIMD the ladder kernel is built for (at most 168 VGPRs; at 128 it spills 13)
#endif

namespace {

// (the plan's type, the argument check, the table entry format, k_seg_combine and k_seg_or_status: msm_seg_shared.h, shared
// with pointset.hip)
constexpr uint32_t SEG_POS = 33;                  // digit positions of a recoded 128-bit magnitude
constexpr uint32_t SEG_TBL = 8;                   // table entries per term: 1 .. 8 times the point
constexpr size_t SEG_ENTRY_BYTES = 64, SEG_PT_WORDS = 27;


// (read at every call, not once per process: tools/msm_segments_time.py and the tests move them between calls of one process;
// the header tells callers not to change them while another thread is inside the library)
uint32_t seg_default_T() {
  const char* e = getenv("S2K_MSM_SEG_T");
  const int t = e ? atoi(e) : S2K_MSM_SEG_T;
  return (uint32_t)(t < 1 ? 1 : (t > (int)SEG_T_MAX ? (int)SEG_T_MAX : t));
}
uint64_t seg_default_crossover() {
  const char* e = getenv("S2K_MSM_SEG_CROSSOVER");
  const long long c = e ? atoll(e) : (long long)S2K_MSM_SEG_CROSSOVER;
  return (uint64_t)(c < 1 ? 1 : c);
}


// The plan.  fill == false: only the counts and the workspace size.
const char* seg_plan_build(size_t n, size_t n_seg, const uint64_t* off, uint32_t T, uint64_t crossover, bool fill, seg_plan& p) {
  if (const char* e = seg_check(n, n_seg, off)) return e;
  p.T = T ? (T > SEG_T_MAX ? SEG_T_MAX : T) : seg_default_T();
  p.crossover = crossover ? crossover : seg_default_crossover();
  T = p.T;
  size_t count_by_len[SEG_T_MAX + 1] = {0};
  if (fill) p.segdesc.assign(2 * n_seg, 0u);
  size_t run_lo = 0, run_hi = 0, run_c = 0;       // the open run of short terms, and the Straus terms in front of it
  for (size_t j = 0; j < n_seg; ++j) {
    const size_t a = (size_t)off[j], L = (size_t)(off[j + 1] - off[j]);
    if ((uint64_t)L > p.crossover) {
      ++p.n_long;
      if (L > p.max_long) p.max_long = L;
      if (fill) {
        p.longs.push_back(j);
        p.segdesc[2 * j] = (uint32_t)p.n_pieces;
        p.segdesc[2 * j + 1] = SEG_LONG;
      }
      if (run_hi > run_lo) { p.runs.push_back(run_lo); p.runs.push_back(run_hi); p.runs.push_back(run_c); }
      run_lo = run_hi = a + L;
      continue;
    }
    const size_t np = (L + T - 1) / T;
    if (fill) {
      p.segdesc[2 * j] = (uint32_t)p.n_pieces;
      p.segdesc[2 * j + 1] = (uint32_t)np;
    }
    if (np) {
      count_by_len[T] += np - 1;
      ++count_by_len[L - (np - 1) * T];
    }
    p.n_pieces += np;
    if (L) {
      if (run_hi == run_lo) { run_lo = a; run_c = p.n_short_terms; }
      run_hi = a + L;
    }
    p.n_short_terms += L;
  }
  if (run_hi > run_lo) { p.runs.push_back(run_lo); p.runs.push_back(run_hi); p.runs.push_back(run_c); }
  // workspace: status word, the segment and piece descriptors, then (only when something runs Straus) digits, tables, piece sums
  size_t o = 0;
  auto carve = [&](size_t bytes) { size_t at = o; o = seg_align(o + bytes, 256); return at; };
  p.piece_stride = seg_align(p.n_pieces, 64);
  p.o_status = carve(256);
  p.o_segdesc = carve(n_seg * 8);
  p.o_pieces = carve(p.n_pieces * 12);
  const size_t span = p.n_short_terms;            // digits and tables are indexed by the term's position among the Straus terms
  p.o_digits = carve(span * 2 * SEG_POS);
  p.o_table = carve(span * SEG_TBL * SEG_ENTRY_BYTES);
  p.o_sums = carve(p.piece_stride * SEG_PT_WORDS * 4);
  p.ws_bytes = o;
  if (!fill) return nullptr;
  // pieces by length, longest first (a stable counting sort: equal lengths stay in segment order)
  size_t start[SEG_T_MAX + 2];
  {
    size_t at = 0;
    for (uint32_t l = T; l >= 1; --l) { start[l] = at; at += count_by_len[l]; }
  }
  p.first.resize(p.n_pieces);
  p.cfirst.resize(p.n_pieces);
  p.len.resize(p.n_pieces);
  p.dest.resize(p.n_pieces);
  size_t id = 0, c = 0;
  for (size_t j = 0; j < n_seg; ++j) {
    const size_t a = (size_t)off[j], L = (size_t)(off[j + 1] - off[j]);
    if ((uint64_t)L > p.crossover) continue;
    for (size_t t = 0; t < L; t += T, ++id) {
      const uint32_t l = (uint32_t)(L - t < T ? L - t : T);
      const size_t at = start[l]++;
      p.first[at] = (uint32_t)(a + t);
      p.cfirst[at] = (uint32_t)(c + t);
      p.len[at] = l;
      p.dest[at] = (uint32_t)id;
    }
    c += L;
  }
  return nullptr;
}

// ---------------------------------------------------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------------------------------------------------

// A magnitude k < 2^128 as 33 signed digits: k + 0x88..8 (32 nibbles of 8) has the nibbles d_p + 8 with d_p in -8 .. 7 and
// k = sum_p d_p 16^p; the 33rd digit is the carry out of bit 128 (0 or 1).  One byte per digit, |d| in the low bits and bit 7
// set when the addend is to be negated (the digit's sign times the sign of the half scalar); a zero digit is the byte 0.
S2K_DEV void seg_store_digits(uint8_t* __restrict__ dg, size_t plane, size_t at, const sc& k, bool neg, bool zero) {
  uint32_t w[5];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    c += (uint64_t)k.v[i] + 0x88888888u;
    w[i] = (uint32_t)c;
    c >>= 32;
  }
  w[4] = (uint32_t)c;
#pragma unroll 1
  for (uint32_t pos = 0; pos < SEG_POS; ++pos) {
    uint32_t word = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) word = (pos >> 3) == (uint32_t)i ? w[i] : word;
    const int nib = (int)((word >> ((pos & 7u) * 4u)) & 15u);
    const int d = pos < 32 ? nib - 8 : nib;
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    const bool flip = (d < 0) != neg;
    dg[(size_t)pos * plane + at] = (zero || mag == 0) ? (uint8_t)0 : (uint8_t)(mag | (flip ? 0x80u : 0u));
  }
}

// terms [lo, lo + count) of the input, the Straus terms [clo, clo + count): digits and table.  NS: the call's Straus terms (plane strides).
__global__ void __launch_bounds__(256)
k_seg_front(uint32_t lo, uint32_t clo, uint32_t count, uint32_t NS, const uint8_t* __restrict__ scalars, const uint8_t* __restrict__ points,
            uint8_t* __restrict__ dg, uint4* __restrict__ tbl, uint32_t* __restrict__ status) {
  const uint32_t id = blockIdx.x * 256 + threadIdx.x;
  if (id >= count) return;
  const size_t i = (size_t)lo + id, c = (size_t)clo + id;
  uint32_t raw[8];
  load_be32(raw, scalars + i * 32);
  const sc k = sc_reduce_once(raw);                     // SetBytes semantics (scalar.go:123)
  const uint8_t* rec = points + i * 65;
  fe29 px, py;
  const uint32_t f = msm_classify_record29(rec, px, py);
  if (f == TERM_MALFORMED) atomicOr(status, 1u);
  sc k1, k2;
  bool neg1, neg2;
  sc_split_glv(k, k1, neg1, k2, neg2);
  const size_t plane = 2 * (size_t)NS;
  seg_store_digits(dg, plane, 2 * c, k1, neg1, f != 1);
  seg_store_digits(dg, plane, 2 * c + 1, k2, neg2, f != 1);
  if (f != 1) return;                                   // (all its digits are zero: the table is never used)
  // the table: entry m - 1 holds m * P.  Jacobian chain 2P, 2P + P, ...: Z_2 from the doubling, Z_{j+1} = Z_j * H_j
  uint4* e = tbl + c * (SEG_TBL * 4);
  seg_entry_store(e, px, py);
  jpt29 cur;
  cur.x = px;
  cur.y = py;
  cur.z = fe29_one();
  cur = jpt29_double(cur);
  seg_entry_store(e + 4, cur.x, cur.y);                 // (parked as they are; made affine below)
  fe29 h[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    cur = jpt29_add_affine(cur, px, py, &h[j]);
    seg_entry_store(e + (size_t)(j + 2) * 4, cur.x, cur.y);
  }
  fe29 zi = fe29_inv_gcd(fe29_normalize_weak(cur.z));   // 1 / Z_8
#pragma unroll
  for (int j = 7; j >= 1; --j) {                        // entry j holds (j + 1) P with Z_{j+1}; zi = 1 / Z_{j+1}
    fe29 X, Y;
    seg_entry_point(seg_entry_fetch(e + (size_t)j * 4), X, Y);
    const fe29 zi2 = fe29_sqr(zi), zi3 = fe29_mul(zi2, zi);
    seg_entry_store(e + (size_t)j * 4, fe29_mul(X, zi2), fe29_mul(Y, zi3));
    if (j >= 2) zi = fe29_mul(zi, h[j - 2]);            // 1 / Z_j = H_{j} / Z_{j+1}  (h[j - 2] took entry j - 1 to entry j)
  }
}


S2K_DEV const uint4* seg_entry_addr(const uint4* __restrict__ tbl, uint32_t first, uint32_t s, uint32_t byte) {
  const uint32_t mag = byte & 15u;
  return tbl + ((size_t)(first + (s >> 1)) * SEG_TBL + (mag ? mag - 1u : 0u)) * 4;
}

__global__ void __launch_bounds__(256, S2K_MSM_SEG_WAVES)
k_seg_ladder(uint32_t npieces, uint32_t NS, const uint32_t* __restrict__ pieces, const uint8_t* __restrict__ dg,
             const uint4* __restrict__ tbl, uint32_t* __restrict__ sums, size_t stride) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npieces) return;
  const uint32_t first = pieces[p] /* among the Straus terms */, steps = 2u * pieces[npieces + p], dest = pieces[2 * (size_t)npieces + p];
  const size_t plane = 2 * (size_t)NS;
  const fe29 beta = seg_beta();
  pt29 acc = pt29_identity();
#pragma unroll 1
  for (int pos = (int)SEG_POS - 1; pos >= 0; --pos) {
    const uint8_t* __restrict__ d = dg + (size_t)pos * plane + 2 * (size_t)first;
    // the first entry of this position and the second digit are asked for in front of the doublings
    uint32_t b_cur = d[0], b_nxt = steps > 1 ? d[1] : 0u;
    seg_raw r_cur = seg_entry_fetch(seg_entry_addr(tbl, first, 0, b_cur));
    if (pos != (int)SEG_POS - 1) {
#pragma unroll 1
      for (int t = 0; t < 4; ++t) acc = pt29_double(acc);
    }
#pragma unroll 1
    for (uint32_t s = 0; s < steps; ++s) {
      fe29 qx, qy;
      seg_entry_point(r_cur, qx, qy);
      // the next entry (a valid address when past the end: this piece's first term) and the digit after it
      const seg_raw r_nxt = seg_entry_fetch(seg_entry_addr(tbl, first, s + 1 < steps ? s + 1 : 0u, b_nxt));
      const uint32_t b_nn = s + 2 < steps ? d[s + 2] : 0u;
      if (b_cur & 15u) {
        if (s & 1u) qx = fe29_mul(qx, beta);                                 // the lambda half: (beta x, y)
        if (b_cur & 0x80u) qy = fe29_normalize_weak(fe29_negate(qy, 1));     // -y at one unit
        acc = pt29_add_mixed(acc, qx, qy);
      }
      r_cur = r_nxt;
      b_cur = b_nxt;
      b_nxt = b_nn;
    }
  }
#pragma unroll
  for (int w = 0; w < 9; ++w) {
    sums[(size_t)w * stride + dest] = acc.x.n[w];
    sums[(size_t)(9 + w) * stride + dest] = acc.y.n[w];
    sums[(size_t)(18 + w) * stride + dest] = acc.z.n[w];
  }
}


}  // namespace

__attribute__((visibility("hidden"))) const char* s2k_internal_seg_plan_build(size_t n, size_t n_seg, const uint64_t* off, uint32_t T,
                                                                               uint64_t crossover, seg_plan& p) {
  return seg_plan_build(n, n_seg, off, T, crossover, true, p);
}

extern "C" {

int s2k_debug_msm_segments_plan(size_t n, size_t n_seg, const uint64_t* seg_offsets, uint32_t piece_terms, uint64_t crossover,
                                uint64_t summary[8], size_t piece_cap, uint32_t* piece_first, uint32_t* piece_len,
                                uint32_t* piece_dest, uint32_t* seg_desc) {
  if (!summary) return fail(nullptr, S2K_ERR_ARG, "null argument");
  seg_plan p;
  const bool fill = piece_first || piece_len || piece_dest || seg_desc;
  if (const char* e = seg_plan_build(n, n_seg, seg_offsets, piece_terms, crossover, fill, p)) return fail(nullptr, S2K_ERR_ARG, "%s", e);
  summary[0] = p.n_pieces;
  summary[1] = p.n_long;
  summary[2] = p.n_short_terms;
  summary[3] = p.ws_bytes;
  summary[4] = p.max_long;
  summary[5] = p.T;
  summary[6] = p.crossover;
  summary[7] = p.runs.size() / 3;
  if (fill) {
    if (piece_cap < p.n_pieces) return fail(nullptr, S2K_ERR_ARG, "piece arrays too small");
    for (size_t i = 0; i < p.n_pieces; ++i) {
      if (piece_first) piece_first[i] = p.first[i];
      if (piece_len) piece_len[i] = p.len[i];
      if (piece_dest) piece_dest[i] = p.dest[i];
    }
    if (seg_desc)
      for (size_t i = 0; i < 2 * n_seg; ++i) seg_desc[i] = p.segdesc[i];
  }
  return S2K_OK;
}

int s2k_multi_scalar_mult_segments_device(s2k_ctx* ctx, size_t n, const void* d_scalars, const void* d_points, size_t n_seg,
                                          const uint64_t* seg_offsets, void* d_out, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n_seg && !d_out) return fail(ctx, S2K_ERR_ARG, "null output buffer");
  if (n && (!d_scalars || !d_points)) return fail(ctx, S2K_ERR_ARG, "null input buffer");
  if (const char* e = seg_check(n, n_seg, seg_offsets)) return fail(ctx, S2K_ERR_ARG, "%s", e);
  if (n_seg == 0) return S2K_OK;
  // one segment on the bucket method is the single-sum call itself: nothing of this file stands in front of it, not even the plan
  if (n_seg == 1 && (uint64_t)n > seg_default_crossover()) return s2k_multi_scalar_mult_device(ctx, n, d_scalars, d_points, d_out, hip_stream);
  seg_plan p;
  if (const char* e = seg_plan_build(n, n_seg, seg_offsets, 0, 0, true, p)) return fail(ctx, S2K_ERR_ARG, "%s", e);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  // both workspaces are brought to their final size before the first launch (growing one frees it)
  rc = ctx_reserve(ctx, &ctx->seg_ws, &ctx->seg_ws_bytes, p.ws_bytes);
  if (rc) return rc;
  for (size_t j : p.longs) {
    rc = s2k_internal_msm_reserve(ctx, (size_t)(seg_offsets[j + 1] - seg_offsets[j]));
    if (rc) return rc;
  }
  uint8_t* ws = (uint8_t*)ctx->seg_ws;
  uint32_t* d_status = (uint32_t*)(ws + p.o_status);
  uint32_t* d_segdesc = (uint32_t*)(ws + p.o_segdesc);
  uint32_t* d_pieces = (uint32_t*)(ws + p.o_pieces);
  uint8_t* d_digits = ws + p.o_digits;
  uint4* d_table = (uint4*)(ws + p.o_table);
  uint32_t* d_sums = (uint32_t*)(ws + p.o_sums);
  const uint8_t* sc_in = (const uint8_t*)d_scalars;
  const uint8_t* pt_in = (const uint8_t*)d_points;
  uint8_t* out = (uint8_t*)d_out;
  HIP_TRY(ctx, hipMemsetAsync(d_status, 0, 256, st));
  if (p.n_long < n_seg) {
    // the plan goes up in ONE copy from a pinned block of the context (segment descriptors and, behind them as in the workspace,
    // the pieces): a copy from pageable memory would make the host wait for everything the caller has queued on the stream.
    // (A call of bucket-method segments alone uploads nothing: only k_seg_combine and the ladder read the plan.)
    const size_t np = p.n_pieces, bytes = (p.o_pieces - p.o_segdesc) + np * 12;
    if (bytes > ctx->seg_host_bytes) {
      if (ctx->seg_host) HIP_TRY(ctx, hipHostFree(ctx->seg_host));
      ctx->seg_host = nullptr;
      ctx->seg_host_bytes = 0;
      HIP_TRY(ctx, hipHostMalloc(&ctx->seg_host, bytes, hipHostMallocDefault));
      ctx->seg_host_bytes = bytes;
    }
    uint8_t* h = (uint8_t*)ctx->seg_host;
    memcpy(h, p.segdesc.data(), n_seg * 8);
    uint32_t* hp = (uint32_t*)(h + (p.o_pieces - p.o_segdesc));
    if (np) {
      memcpy(hp, p.cfirst.data(), np * 4);
      memcpy(hp + np, p.len.data(), np * 4);
      memcpy(hp + 2 * np, p.dest.data(), np * 4);
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_segdesc, h, bytes, hipMemcpyHostToDevice, st));
  }
  if (p.n_pieces) {
    const size_t np = p.n_pieces;
    for (size_t r = 0; r < p.runs.size(); r += 3) {     // (one launch per run of short segments: at most one more than there are long ones)
      const size_t lo = p.runs[r], cnt = p.runs[r + 1] - lo;
      k_seg_front<<<blocks_for(cnt), 256, 0, st>>>((uint32_t)lo, (uint32_t)p.runs[r + 2], (uint32_t)cnt, (uint32_t)p.n_short_terms, sc_in, pt_in,
                                                     d_digits, d_table, d_status);
    }
    HIP_TRY(ctx, hipGetLastError());
    k_seg_ladder<<<blocks_for(np), 256, 0, st>>>((uint32_t)np, (uint32_t)p.n_short_terms, d_pieces, d_digits, d_table, d_sums, p.piece_stride);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (p.n_long < n_seg) {
    k_seg_combine<<<blocks_for(n_seg), 256, 0, st>>>((uint32_t)n_seg, d_segdesc, d_sums, p.piece_stride, out);
    HIP_TRY(ctx, hipGetLastError());
  }
  for (size_t j : p.longs) {                            // the bucket method, one segment at a time, no synchronisation between them
    const size_t a = (size_t)seg_offsets[j], L = (size_t)(seg_offsets[j + 1] - seg_offsets[j]);
    uint32_t* d_st = nullptr;
    rc = s2k_internal_msm_enqueue(ctx, st, L, sc_in + a * 32, pt_in + a * 65, out + j * 65, &d_st);
    if (rc) return rc;
    k_seg_or_status<<<1, 1, 0, st>>>(d_st, d_status);
    HIP_TRY(ctx, hipGetLastError());
  }
  // malformed point records are a caller error (the reference cannot even construct such Points)
  uint32_t h_status = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&h_status, d_status, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;   // the stream has been synchronised: nothing of this context is in flight
  if (h_status) return fail(ctx, S2K_ERR_ARG, "malformed point record in multi-scalar multiplication input");
  return S2K_OK;
}

int s2k_multi_scalar_mult_segments(s2k_ctx* ctx, size_t n, const uint8_t* scalars, const uint8_t* points, size_t n_seg,
                                   const uint64_t* seg_offsets, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n_seg && !out) return fail(ctx, S2K_ERR_ARG, "null output buffer");
  if (n && (!scalars || !points)) return fail(ctx, S2K_ERR_ARG, "null input buffer");
  if (const char* e = seg_check(n, n_seg, seg_offsets)) return fail(ctx, S2K_ERR_ARG, "%s", e);
  if (n_seg == 0) return S2K_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  const size_t sizes[3] = {n * 32 + 16, n * 65 + 16, n_seg * 65 + 16};
  uint8_t* d[3];
  rc = ctx_stage(ctx, sizes, 3, d);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  s2k_phase_guard phase(ctx->device, n * 97);            // (two verifiers on two threads: engine_internal.h)
  if (n) {
    HIP_TRY(ctx, hipMemcpyAsync(d[0], scalars, n * 32, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d[1], points, n * 65, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(ctx, phase.landed(st));
  rc = s2k_multi_scalar_mult_segments_device(ctx, n, d[0], d[1], n_seg, seg_offsets, d[2], st);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out, d[2], n_seg * 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return S2K_OK;
}

}  // extern "C"
