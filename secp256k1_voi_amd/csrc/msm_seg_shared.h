// msm_seg_shared.h — what the two segmented multiscalar calls share (msm_seg.hip: points given per term; pointset.hip: points
// named by index into a point set): the argument check, the host plan (built in msm_seg.hip), the 64-byte table entry format,
// the piece sums and the combine kernel.  The device code has internal linkage: each translation unit has its own copy.
#pragma once
#include <vector>

#include "engine_internal.h"
#include "fe29_inv.h"
#include "pt29.h"

constexpr size_t SEG_MAX_TERMS = 0x1fffffffu;     // the limit s2k_multi_scalar_mult_device enforces
constexpr uint32_t SEG_T_MAX = 64;
constexpr uint32_t SEG_LONG = 0x80000000u;        // in the piece count of a segment: it takes the bucket method

struct seg_plan {
  uint32_t T = 0;
  uint64_t crossover = 0;
  size_t n_pieces = 0, n_long = 0, n_short_terms = 0, max_long = 0;
  std::vector<uint32_t> first, len, dest;         // pieces in launch order (longest first); dest: index in segment order
  std::vector<uint32_t> cfirst;                   // the piece's first term counted among the Straus terms only (digits, tables)
  std::vector<uint32_t> segdesc;                  // per segment: first piece (segment order), piece count or SEG_LONG
  std::vector<size_t> runs;                       // maximal runs of terms of short segments: lo, hi, position of lo among the Straus terms
  std::vector<size_t> longs;                      // the segments that take the bucket method
  // workspace
  size_t o_status = 0, o_segdesc = 0, o_pieces = 0, o_digits = 0, o_table = 0, o_sums = 0, ws_bytes = 0, piece_stride = 0;
};

inline size_t seg_align(size_t x, size_t a) { return (x + a - 1) / a * a; }

// nullptr: the arguments are fine
inline const char* seg_check(size_t n, size_t n_seg, const uint64_t* off) {
  if (n > SEG_MAX_TERMS) return "batch too large";
  if (n_seg > SEG_MAX_TERMS) return "too many segments";
  if (!off) return n_seg == 0 && n == 0 ? nullptr : "null segment offsets";
  if (off[0] != 0) return "segment offsets do not start at 0";
  for (size_t j = 0; j < n_seg; ++j) {
    if (off[j + 1] > (uint64_t)n) return "segment offset beyond the number of terms";     // (64-bit: never cut to 32 bits)
    if (off[j + 1] < off[j]) return "segment offsets decrease";
  }
  if (off[n_seg] != (uint64_t)n) return "segment offsets do not end at the number of terms";
  return nullptr;
}

// msm_seg.hip: the plan for pieces of T terms and the given crossover, filled (0: that call's own defaults).  nullptr: fine.
const char* s2k_internal_seg_plan_build(size_t n, size_t n_seg, const uint64_t* off, uint32_t T, uint64_t crossover, seg_plan& p);

namespace {

S2K_DEV void seg_entry_store(uint4* __restrict__ e, const fe29& x, const fe29& y) {   // canonical words, 64 bytes
  uint32_t xw[8], yw[8];
  fe29_to_words(xw, fe29_normalize(x));
  fe29_to_words(yw, fe29_normalize(y));
  e[0] = make_uint4(xw[0], xw[1], xw[2], xw[3]);
  e[1] = make_uint4(xw[4], xw[5], xw[6], xw[7]);
  e[2] = make_uint4(yw[0], yw[1], yw[2], yw[3]);
  e[3] = make_uint4(yw[4], yw[5], yw[6], yw[7]);
}
struct seg_raw {
  uint4 a, b, c, d;
};
S2K_DEV seg_raw seg_entry_fetch(const uint4* __restrict__ e) {
  seg_raw r;
  r.a = e[0]; r.b = e[1]; r.c = e[2]; r.d = e[3];
  return r;
}
S2K_DEV void seg_entry_point(const seg_raw& r, fe29& x, fe29& y) {
  const uint32_t xw[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w}, yw[8] = {r.c.x, r.c.y, r.c.z, r.c.w, r.d.x, r.d.y, r.d.z, r.d.w};
  x = fe29_from_words(xw);
  y = fe29_from_words(yw);
}

S2K_DEV fe29 seg_beta() { return fe29_from_words(FE_BETA); }

S2K_DEV pt29 seg_sum_load(const uint32_t* __restrict__ sums, size_t stride, size_t slot) {
  pt29 r;
#pragma unroll
  for (int w = 0; w < 9; ++w) {
    r.x.n[w] = sums[(size_t)w * stride + slot];
    r.y.n[w] = sums[(size_t)(9 + w) * stride + slot];
    r.z.n[w] = sums[(size_t)(18 + w) * stride + slot];
  }
  return r;
}

__global__ void __launch_bounds__(256)
k_seg_combine(uint32_t n_seg, const uint32_t* __restrict__ segdesc, const uint32_t* __restrict__ sums, size_t stride,
              uint8_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_seg) return;
  const uint32_t p0 = segdesc[2 * (size_t)j], np = segdesc[2 * (size_t)j + 1];
  if (np & SEG_LONG) return;                            // the bucket method writes this record
  uint8_t* o = out + (size_t)j * 65;
  pt29 acc = pt29_identity();
  if (np) acc = seg_sum_load(sums, stride, p0);
#pragma unroll 1
  for (uint32_t t = 1; t < np; ++t) acc = pt29_add(acc, seg_sum_load(sums, stride, (size_t)p0 + t));
  if (fe29_is_zero(acc.z)) {
    for (int i = 0; i < 65; ++i) o[i] = 0;
    return;
  }
  const fe29 zi = fe29_inv_gcd(fe29_normalize_weak(acc.z));
  uint32_t xw[8], yw[8];
  fe29_to_words(xw, fe29_normalize(fe29_mul(acc.x, zi)));
  fe29_to_words(yw, fe29_normalize(fe29_mul(acc.y, zi)));
  o[0] = 0x04;
  store_be32_unaligned(o + 1, xw);
  store_be32_unaligned(o + 33, yw);
}

__global__ void k_seg_or_status(const uint32_t* __restrict__ from, uint32_t* __restrict__ to) {
  if (*from) atomicOr(to, *from);
}

}  // namespace
