// msm_terms.h — the term format of the multiscalar core (msm.hip), device side: what a front end writes and the core reads.
//
// A term array for N terms is
//   scw   [SCW_WORDS][N] planes: the 128-bit magnitude of term t in scw[w * N + t], w < 4, and one zero plane
//   ptw   [N][TERM_REC_WORDS]: a 64-byte record per term, x then y as canonical words, y already negated where the term is
//   flag  [N]: TERM_SKIP / TERM_FINITE / TERM_MALFORMED
// Its writers are msm_store_term / msm_store_split (a front end that has a scalar and a point), msm_copy_term (the whole-batch
// verifiers' bisection, rlc.hip) and nothing else.  msm_classify_record / msm_classify_record29 are the rule for a 65-byte input
// record: k_msm_parse, k_seg_front (msm_seg.hip) and k_ps_chain (pointset.hip) call them.  The test hook's k_msm_debug_fill
// (msm.hip) has a stricter rule of its own for the identity.
#pragma once
#include "fe29.h"
#include "sc.h"

constexpr int SCW_WORDS = 5;        // scalar planes per term: 128-bit magnitude + one zero word
constexpr int TERM_REC_WORDS = 16;  // words of a term's point record
// flag of a term, and of the 65-byte record it came from
enum : uint8_t {
  TERM_SKIP = 0,       // the identity (an input record that starts 0x00), or a term its front end left out of the sum
  TERM_FINITE = 1,     // a point on the curve
  TERM_MALFORMED = 2   // a record that is neither: the call's status word says so
};

// term `t` of a term array with plane stride N: magnitude k (< 2^128), point (x, +-y)
S2K_DEV void msm_store_term(uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw, size_t N, size_t t, const sc& k,
                            const uint32_t x[8], const uint32_t y[8], bool neg) {
#pragma unroll
  for (int w = 0; w < SCW_WORDS - 1; ++w) scw[(size_t)w * N + t] = k.v[w];
  scw[(size_t)(SCW_WORDS - 1) * N + t] = 0;
  uint32_t ny[8];
  u256_sub(ny, FE_P, y);                                   // y != 0 on this curve
  // points as 64-byte records [t][16 words]: the bucket pass gathers them by index, one
  // contiguous record per lane (planes would cost 16 sparse sectors per gathered point)
  uint4* rec4 = reinterpret_cast<uint4*>(ptw + t * TERM_REC_WORDS);
  rec4[0] = make_uint4(x[0], x[1], x[2], x[3]);
  rec4[1] = make_uint4(x[4], x[5], x[6], x[7]);
  rec4[2] = neg ? make_uint4(ny[0], ny[1], ny[2], ny[3]) : make_uint4(y[0], y[1], y[2], y[3]);
  rec4[3] = neg ? make_uint4(ny[4], ny[5], ny[6], ny[7]) : make_uint4(y[4], y[5], y[6], y[7]);
}
// k * (x, y) -> terms t1, t2:  |k1| * (x, +-y) and |k2| * (beta x, +-y)   (mulBeta, point_mul_glv.go:191)
S2K_DEV void msm_store_split(uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw, size_t N, size_t t1, size_t t2,
                             const sc& k, const uint32_t x[8], const uint32_t y[8]) {
  sc k1, k2;
  bool neg1, neg2;
  sc_split_glv(k, k1, neg1, k2, neg2);
  msm_store_term(scw, ptw, N, t1, k1, x, y, neg1);
  uint32_t bx[8];
  fe29_to_words(bx, fe29_normalize(fe29_mul(fe29_from_words(x), fe29_from_words(FE_BETA))));
  msm_store_term(scw, ptw, N, t2, k2, bx, y, neg2);
}
// term `src` of the arrays (s_scw, s_ptw), plane stride NS -> term `dst` of (scw, ptw), plane stride N: the magnitude planes,
// the record as four uint4, and the zero plane where the destination has one (ZERO_PLANE: the kept terms of rlc.hip do not)
template <bool ZERO_PLANE>
S2K_DEV void msm_copy_term(uint32_t* __restrict__ scw, uint32_t* __restrict__ ptw, size_t N, size_t dst,
                           const uint32_t* __restrict__ s_scw, const uint32_t* __restrict__ s_ptw, size_t NS, size_t src) {
#pragma unroll
  for (int w = 0; w < SCW_WORDS - 1; ++w) scw[(size_t)w * N + dst] = s_scw[(size_t)w * NS + src];
  if constexpr (ZERO_PLANE) scw[(size_t)(SCW_WORDS - 1) * N + dst] = 0;
  const uint4* a = reinterpret_cast<const uint4*>(s_ptw + src * TERM_REC_WORDS);
  uint4* b = reinterpret_cast<uint4*>(ptw + dst * TERM_REC_WORDS);
  b[0] = a[0]; b[1] = a[1]; b[2] = a[2]; b[3] = a[3];
}

// (x, y) canonical and y^2 == x^3 + 7 on the 9x29 field (a third of the instructions of the 8x32 form): the point check of
// a record (xyOnCurve, point_s11n.go:298-307) and NewPublicKey's validation of an X || Y key (secec.go:188-216)
// (xy_on_curve29: x, y receive the coordinates as field elements when both are canonical, and are left alone otherwise)
S2K_DEV bool xy_on_curve29(fe29& x, fe29& y, const uint32_t xw[8], const uint32_t yw[8]) {
  bool on = fe_is_canonical_raw(xw) && fe_is_canonical_raw(yw);
  if (on) {
    x = fe29_from_words(xw);
    y = fe29_from_words(yw);
    fe29 rhs = fe29_mul(fe29_sqr(x), x);
    rhs.n[0] += 7;
    on = fe29_eq(fe29_sqr(y), rhs);
  }
  return on;
}
S2K_DEV bool xy_on_curve_words(const uint32_t xw[8], const uint32_t yw[8]) {
  fe29 x, y;
  return xy_on_curve29(x, y, xw, yw);
}
// A 65-byte point record -> its flag: 0x04 || X || Y with both coordinates canonical and on the curve is TERM_FINITE, a record
// that starts 0x00 is the identity (TERM_SKIP; only byte 0 is looked at), anything else is TERM_MALFORMED.  The caller raises
// its own status bit for a malformed record.  Two forms, by what the caller goes on with (each kernel's machine code is what
// it was when the kernel had the rule written out):
// msm_classify_record29: the point as field elements (msm_seg.hip, pointset.hip) - px, py receive the coordinates of a record
// that starts 0x04 with both canonical, and zero otherwise;
S2K_DEV uint32_t msm_classify_record29(const uint8_t* rec, fe29& px, fe29& py) {
  uint32_t f = TERM_SKIP;
  px = fe29_zero();
  py = fe29_zero();
  if (rec[0] == 0x04) {
    uint32_t xw[8], yw[8];
    load_be32_unaligned(xw, rec + 1);
    load_be32_unaligned(yw, rec + 33);
    f = xy_on_curve29(px, py, xw, yw) ? TERM_FINITE : TERM_MALFORMED;
  } else if (rec[0] != 0x00) {
    f = TERM_MALFORMED;
  }
  return f;
}
// msm_classify_record: the point as words, for msm_store_split (k_msm_parse) - xw, yw receive the coordinates of a record that
// starts 0x04, and zeros otherwise.
S2K_DEV uint8_t msm_classify_record(const uint8_t* rec, uint32_t xw[8], uint32_t yw[8]) {
  uint8_t f = TERM_SKIP;
#pragma unroll
  for (int w = 0; w < 8; ++w) xw[w] = 0;
#pragma unroll
  for (int w = 0; w < 8; ++w) yw[w] = 0;
  if (rec[0] == 0x04) {
    load_be32_unaligned(xw, rec + 1);
    load_be32_unaligned(yw, rec + 33);
    f = xy_on_curve_words(xw, yw) ? TERM_FINITE : TERM_MALFORMED;
  } else if (rec[0] != 0x00) {
    f = TERM_MALFORMED;
  }
  return f;
}
