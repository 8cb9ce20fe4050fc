// h2c.hip — hashing to the curve, RFC 9380 for secp256k1 (suites secp256k1_XMD:SHA-256_SSWU_RO_ / _NU_), batched: what the
// reference's secec/h2c package computes one message at a time (h2c.go:25-63, h2c_expand_message.go:27-139,
// point_h2c.go:23-55, internal/swu/swu.go:70-199, internal/field/field_reduce.go:24-64).  One lane per item, 256-thread
// blocks, no LDS.  Public data only, variable time.
//
// The reference inverts seven times and runs two square-root chains per hash_to_curve.  Here a mapped point costs ONE
// exponentiation (sqrt_ratio for p = 3 mod 4, RFC 9380 F.2.1.2: fe29_pow_p34) and a record ONE inversion: the SSWU
// x-coordinate stays a fraction xn / xd, the 3-isogeny is evaluated on that fraction into a projective point, the two
// points of the RO suite meet in the complete projective addition, and only the record's Z is inverted.
//
// Units of the lazy 9x29 field are in [brackets] (fe29.h: a value has w units when limbs 0..7 are <= w * 2^29 and limb 8
// <= w * (2^24 + 16); a product needs the units of its operands, summed over fused terms, to multiply to <= 7.8, gives [1];
// add sums; negate(a, w) gives [w + 1]).  Constants are canonical: [1].
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "engine_internal.h"
#include "fe29.h"
#include "h2c_host.h"
#include "pt29.h"
#include "sha256.h"

using namespace s2k;

namespace {

// DST_prime as the kernels read it: device memory behind the call's status word (s2k_ctx::h2c_dev)
struct h2c_dstp {
  uint32_t len;       // 2 .. 256
  uint8_t b[256];
};
constexpr size_t H2C_DSTP_OFF = 16, H2C_BLOCK_BYTES = 512;
static_assert(H2C_DSTP_OFF + sizeof(h2c_dstp) <= H2C_BLOCK_BYTES, "block layout");

struct sha_words {
  uint32_t w[8];
};

// SHA-256 state after the 64 zero bytes of Z_pad (msg_prime = Z_pad || msg || ..., h2c_expand_message.go:76): a constant,
// so b_0 starts from it (re-derived by tests/test_h2c_model.py)
__device__ static const uint32_t H2C_ZPAD_MIDSTATE[8] = {0xda5698beu, 0x17b9b469u, 0x62335799u, 0x779fbecau,
                                                         0x8ce5d491u, 0xc0d26243u, 0xbafef9eau, 0x1837a9d8u};

#define H2C_CONST(name, ...) \
  S2K_DEV fe29 name() { return fe29{{__VA_ARGS__}}; }
// A' of E': y^2 = x^3 + A'x + 1771 (swu.go:22-26), Z = -11 (:16-20), c2 = sqrt(-Z) = sqrt(11), the isogeny's k_(i,j)
// (:28-65; RFC 9380 E.1) and 2^256 mod p = 2^32 + 977, as canonical 29-bit limbs
H2C_CONST(H2C_A, 0x1a444533u, 0x02a23e00u, 0x1bc39750u, 0x07a6c796u, 0x1d272e95u, 0x0aac787au, 0x0b728229u, 0x157bacc3u, 0x003f8731u)
H2C_CONST(H2C_Z, 0x1ffffc24u, 0x1ffffff7u, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x00ffffffu)
H2C_CONST(H2C_C2, 0x103c4a59u, 0x03394e41u, 0x11e2774au, 0x109e014eu, 0x02afeec1u, 0x1fd9c7c2u, 0x0f95eb44u, 0x004e4802u, 0x0031fdf3u)
H2C_CONST(H2C_K10, 0x0aaaa8c7u, 0x11c71c6du, 0x038e38e3u, 0x071c71c7u, 0x0e38e38eu, 0x1c71c71cu, 0x18e38e38u, 0x11c71c71u, 0x008e38e3u)
H2C_CONST(H2C_K11, 0x117c6581u, 0x1ff88227u, 0x1d8ee4b7u, 0x0ba5f817u, 0x144c5d59u, 0x0ae753feu, 0x0756e7ccu, 0x19017864u, 0x0007d3d4u)
H2C_CONST(H2C_K12, 0x1d9dd262u, 0x165e85a9u, 0x1f100c53u, 0x00c28806u, 0x1caece45u, 0x09ef6512u, 0x139b8a90u, 0x11a47e46u, 0x00534c32u)
H2C_CONST(H2C_K13, 0x0aaaa88cu, 0x11c71c6du, 0x038e38e3u, 0x071c71c7u, 0x0e38e38eu, 0x1c71c71cu, 0x18e38e38u, 0x11c71c71u, 0x008e38e3u)
H2C_CONST(H2C_K20, 0x181eb49bu, 0x1f35ba2bu, 0x1e121f67u, 0x1a812a85u, 0x040dd86cu, 0x0665dbdbu, 0x062a728du, 0x0327b292u, 0x00d35771u)
H2C_CONST(H2C_K21, 0x0a8c6d14u, 0x0952b309u, 0x17906ef1u, 0x06d6c83eu, 0x0225406du, 0x196a8daau, 0x1077df12u, 0x1ec8707bu, 0x00edadc6u)
H2C_CONST(H2C_K30, 0x0e38e23cu, 0x097b425cu, 0x1da12f68u, 0x1097b425u, 0x0bda12f6u, 0x0d097b42u, 0x04bda12fu, 0x1ed097b4u, 0x004bda12u)
H2C_CONST(H2C_K31, 0x001d71a3u, 0x1fe487e1u, 0x01b69bf7u, 0x15608dadu, 0x0a6d5647u, 0x12a58950u, 0x103ea742u, 0x065ab96fu, 0x00c75e0cu)
H2C_CONST(H2C_K32, 0x1ecee931u, 0x1b2f42d4u, 0x0f880629u, 0x10614403u, 0x0e576722u, 0x04f7b289u, 0x09cdc548u, 0x08d23f23u, 0x0029a619u)
H2C_CONST(H2C_K33, 0x18e38d84u, 0x05ed0979u, 0x1684bda1u, 0x025ed097u, 0x0f684bdau, 0x1425ed09u, 0x12f684bdu, 0x1b425ed0u, 0x002f684bu)
H2C_CONST(H2C_K40, 0x1ffff93bu, 0x1ffffff7u, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x00ffffffu)
H2C_CONST(H2C_K41, 0x085c2573u, 0x1da12e93u, 0x1a365e37u, 0x0f837f91u, 0x0c298946u, 0x13319391u, 0x127f57a7u, 0x097717b6u, 0x007a0653u)
H2C_CONST(H2C_K42, 0x1fd2a76fu, 0x1dfc0c95u, 0x0358a669u, 0x1a422c5eu, 0x0337e0a3u, 0x061fd47fu, 0x08b3ce9cu, 0x0e2ca8b9u, 0x006484aau)
H2C_CONST(H2C_R256, 0x000003d1u, 0x00000008u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u)
constexpr uint32_t H2C_B = 1771;   // B' (swu.go:25-26)

// ---------------------------------------------------------------------------------------
// expand_message_xmd (h2c_expand_message.go:75-136)
// ---------------------------------------------------------------------------------------
// One SHA-256 of  head || msg[0 .. mlen) || tail || DST_prime  continued from state `st`, which has taken `prior` bytes
// (0, or 64 for the Z_pad block).  head: the 32 bytes of `head` as big-endian words (has_head) or nothing; tail: the top
// `tlen` <= 3 bytes of `tail`.  The message is read by bytes: any length, any alignment; msg is not touched when mlen == 0.
__device__ __noinline__ sha_words xmd_hash(sha_words st, uint32_t prior, sha_words head, bool has_head,
                                           const uint8_t* __restrict__ msg, uint64_t mlen, uint32_t tail, uint32_t tlen,
                                           const h2c_dstp* __restrict__ dp) {
  const uint32_t dlen = dp->len;
  const uint64_t head_len = has_head ? 32u : 0u;
  const uint64_t o_tail = head_len + mlen, o_dst = o_tail + tlen, total = o_dst + dlen;
  const uint64_t bits = ((uint64_t)prior + total) * 8;
  const uint64_t nblocks = (total + 9 + 63) / 64;        // 0x80, zeros, 64-bit big-endian bit count
#pragma unroll 1
  for (uint64_t blk = 0; blk < nblocks; ++blk) {
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      uint32_t word = 0;
      if (i < 8 && has_head && blk == 0) {
        word = head.w[i];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint64_t pos = blk * 64 + (uint64_t)(i * 4 + j);      // >= head_len here
          uint32_t byte;
          if (pos < o_tail) byte = msg[pos - head_len];
          else if (pos < o_dst) byte = (tail >> (24u - 8u * (uint32_t)(pos - o_tail))) & 0xffu;
          else if (pos < total) byte = dp->b[pos - o_dst];
          else byte = pos == total ? 0x80u : 0u;
          word = (word << 8) | byte;
        }
      }
      w[i] = word;
    }
    if (blk == nblocks - 1) {
      w[14] = (uint32_t)(bits >> 32);
      w[15] = (uint32_t)bits;
    }
    sha256_compress(st.w, w);
  }
  return st;
}

S2K_DEV sha_words sha_iv() {
  sha_words r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.w[i] = SHA256_IV[i];
  return r;
}
// b_0 = H(Z_pad || msg || I2OSP(len_in_bytes, 2) || I2OSP(0, 1) || DST_prime)  (:75-81)
S2K_DEV sha_words xmd_b0(const uint8_t* msg, uint64_t mlen, uint32_t len_in_bytes, const h2c_dstp* dp) {
  sha_words st;
#pragma unroll
  for (int i = 0; i < 8; ++i) st.w[i] = H2C_ZPAD_MIDSTATE[i];
  return xmd_hash(st, 64, st, false, msg, mlen, len_in_bytes << 16, 3, dp);
}
// b_i = H(strxor(b_0, b_(i-1)) || I2OSP(i, 1) || DST_prime), b_1 with b_0 itself  (:83-89, :116-125)
S2K_DEV sha_words xmd_bi(const sha_words& b0, const sha_words& prev, uint32_t i, const h2c_dstp* dp) {
  sha_words head;
#pragma unroll
  for (int k = 0; k < 8; ++k) head.w[k] = i == 1 ? b0.w[k] : (b0.w[k] ^ prev.w[k]);
  return xmd_hash(sha_iv(), 0, head, true, nullptr, 0, i << 24, 1, dp);
}

// The byte range of item idx, checked against the message buffer: false for a range that decreases or leaves [0, total)
// (and for offsets that do not start at 0); nothing outside the offsets array's n + 1 entries is read.
S2K_DEV bool h2c_msg_range(uint64_t& lo, uint64_t& hi, size_t idx, const uint64_t* __restrict__ offs, uint64_t msg_len, uint64_t total) {
  if (offs) {
    lo = offs[idx];
    hi = offs[idx + 1];
    if (idx == 0 && lo != 0) return false;
  } else {
    lo = (uint64_t)idx * msg_len;       // (n * msg_len <= total was checked on the host)
    hi = lo + msg_len;
  }
  return lo <= hi && hi <= total;
}

// ---------------------------------------------------------------------------------------
// hash_to_field, simplified SWU, 3-isogeny
// ---------------------------------------------------------------------------------------
// OS2IP(hi || lo) mod p for hi < 2^256 (zero-extended), lo < 2^256, both as little-endian words: lo + hi * 2^256 with
// 2^256 = 2^32 + 977 (mod p), as field operations (field.Element.SetWideBytes, field_reduce.go:24-64, does it with 2^192
// and 2^384).  fe29_from_words gives limbs 0..7 < 2^29 and limb 8 < 2^24 for ANY 256-bit value, so lo >= p is just another
// representative: [1].  hi [1] * R256 [1] + lo [1] through one reduction -> [1].
S2K_DEV fe29 h2c_wide_reduce(const uint32_t hi[8], const uint32_t lo[8]) {
  return fe29_mul_plus(fe29_from_words(hi), H2C_R256(), fe29_from_words(lo));
}

// map_to_curve for one field element u [1]: map_to_curve_simple_swu in the straight-line form of RFC 9380 F.2 (the
// reference's swu.go:70-153 without its step 25, the inversion: x stays xn / xd), then the 3-isogeny (swu.go:155-199) on
// that fraction.  Result: a projective point of secp256k1 with x, y, z [1].
__device__ __noinline__ pt29 h2c_map_to_curve(fe29 u) {
  // ---- SSWU on E' ----
  fe29 uu = fe29_sqr(u);                                                       // [1]
  fe29 tv1 = fe29_negate(fe29_mul_small_norm(uu, 11), 1);                      // [2]   Z u^2 (steps 1-2)
  fe29 tv2 = fe29_sqr_plus(tv1, tv1);                                          // [2]^2 + [2] -> [1]   tv1^2 + tv1 (3-4)
  // B (tv2 + 1): the +1 lands on limb 0 (< 2^29 + 1); times 1771 < 2^11 the carries stay below 2^12 and the fold of bit
  // 256 adds < 2^22 to limb 0: [1] in the sense of fe29_mul_small_norm's own result (5-6)
  fe29 tv3 = fe29_mul_small_norm(fe29_add(tv2, fe29_one()), H2C_B);            // [1]
  // tv4 = A * (tv2 != 0 ? -tv2 : Z): the exceptional branch, reached by u = 0 and by Z u^2 = -1 (7-8)
  const bool exceptional = fe29_is_zero(tv2);
  fe29 xd = fe29_mul(H2C_A(), fe29_select(exceptional, fe29_negate(tv2, 1), H2C_Z()));   // [1]*[2] -> [1]   tv4
  fe29 s3 = fe29_sqr(tv3), s4 = fe29_sqr(xd);                                  // [1]
  fe29 a4 = fe29_mul_plus(H2C_A(), s4, s3);                                    // [1]*[1] + [1] -> [1]   tv3^2 + A tv4^2 (9-12)
  fe29 v = fe29_mul(s4, xd);                                                   // [1]   tv6 = tv4^3 (14)
  fe29 gn = fe29_mul_plus(a4, tv3, fe29_mul_small_norm(v, H2C_B));             // [1]*[1] + [1] -> [1]   (13, 15-16): g(x1) = gn / v
  // sqrt_ratio(gn, v), F.2.1.2 (18): y1 = (gn v^3)^((p-3)/4) * gn v; a square root of gn / v when there is one
  fe29 gv = fe29_mul(gn, v);                                                   // [1]
  fe29 y1 = fe29_mul(fe29_pow_p34(fe29_mul(fe29_sqr(v), gv)), gv);             // [1]
  const bool is_square = fe29_eq(fe29_mul(fe29_sqr(y1), v), gn);               // y1^2 v == gn   (gn [1])
  // the other branch: x2 = tv1 x1 and y = tv1 u y1 sqrt(-Z), a root of g(x2) (17, 19-20)
  fe29 x2n = fe29_mul(tv1, tv3);                                               // [2]*[1] -> [1]
  fe29 y2 = fe29_mul(fe29_mul(tv1, u), fe29_mul(y1, H2C_C2()));                // [1]*[1] -> [1]
  fe29 xn = fe29_select(is_square, x2n, tv3);                                  // [1]   (21)
  fe29 y = fe29_select(is_square, y2, y1);                                     // [1]   (22)
  const uint32_t sgn_u = fe29_normalize(u).n[0] & 1u, sgn_y = fe29_normalize(y).n[0] & 1u;
  y = fe29_cond_negate1(y, sgn_u != sgn_y);                                    // [2]   (23-24)
  // ---- 3-isogeny on x' = xn / xd (swu.go:155-199), every polynomial scaled to a common power of xd ----
  fe29 n2 = fe29_sqr(xn), d2 = fe29_sqr(xd), nd = fe29_mul(xn, xd);            // [1]
  fe29 n3 = fe29_mul(n2, xn), d3 = fe29_mul(d2, xd);                           // [1]
  fe29 n2d = fe29_mul(n2, xd), nd2 = fe29_mul(xn, d2);                         // [1]
  // x_num xd^3, x_den xd^2, y_num xd^3, y_den xd^3: sums of two fused pairs, each pair [1]*[1] + [1]*[1] -> [1]
  fe29 nx = fe29_add(fe29_mul_add_mul(H2C_K13(), n3, H2C_K12(), n2d), fe29_mul_add_mul(H2C_K11(), nd2, H2C_K10(), d3));   // [2]
  fe29 dx = fe29_add(fe29_mul_add_mul(H2C_K21(), nd, H2C_K20(), d2), n2);                                                 // [2]
  fe29 ny = fe29_add(fe29_mul_add_mul(H2C_K33(), n3, H2C_K32(), n2d), fe29_mul_add_mul(H2C_K31(), nd2, H2C_K30(), d3));   // [2]
  fe29 dy = fe29_add(fe29_mul_add_mul(H2C_K42(), n2d, H2C_K41(), nd2), fe29_mul_plus(H2C_K40(), d3, n3));                 // [2]
  // x = nx / (dx xd), y = y' ny / dy  ->  (nx dy : y' ny dx xd : dx xd dy)
  fe29 zx = fe29_mul(dx, xd);                                                  // [2]*[1] -> [1]
  pt29 r;
  r.x = fe29_mul(nx, dy);                                                      // [2]*[2] -> [1]
  r.y = fe29_mul(fe29_mul(y, ny), zx);                                         // [2]*[2] -> [1], [1]*[1] -> [1]
  r.z = fe29_mul(zx, dy);                                                      // [1]*[2] -> [1]
  // IsoMap's identity result (a vanishing denominator, point_h2c.go:48-52).  Dead for an SSWU output: xd = tv4 is never
  // zero, x_den has the double root x0 = 0x89291c84...6ab9c5a5 at which y_den vanishes too, and g'(x0) is a non-square,
  // so no point of E'(F_p) has that x.  Kept as the reference keeps it: two selects.
  const bool at_infinity = fe29_is_zero(r.z);
  r.x = fe29_select(at_infinity, r.x, fe29_zero());
  r.y = fe29_select(at_infinity, r.y, fe29_one());
  return r;
}

// the record of a projective point (x, y, z [1]): the call's one inversion; 65 zero bytes for the identity
S2K_DEV void h2c_store(uint8_t* __restrict__ rec, const pt29& p) {
  if (fe29_is_zero(p.z)) {
    for (int i = 0; i < 65; ++i) rec[i] = 0;
    return;
  }
  const fe29 zi = fe29_inv(p.z);                                               // [1] -> [1]
  uint32_t xw[8], yw[8];
  fe29_to_words(xw, fe29_normalize(fe29_mul(p.x, zi)));
  fe29_to_words(yw, fe29_normalize(fe29_mul(p.y, zi)));
  rec[0] = 0x04;
  store_be32_unaligned(rec + 1, xw);
  store_be32_unaligned(rec + 33, yw);
}

// ---------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------
// message bytes -> record: hash_to_field with expand_message_xmd (48 bytes per element: b_1 .. b_2 for one, b_1 .. b_3
// for two), map_to_curve each, the complete addition for two, one record
__global__ void __launch_bounds__(256)
k_h2c_hash(uint32_t n, uint32_t count, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint64_t msg_len,
           uint64_t total, const h2c_dstp* __restrict__ dp, uint8_t* __restrict__ out, uint32_t* __restrict__ status) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  uint8_t* rec = out + idx * 65;
  uint64_t lo, hi;
  if (!h2c_msg_range(lo, hi, idx, offs, msg_len, total)) {
    atomicOr(status, 1u);
    for (int i = 0; i < 65; ++i) rec[i] = 0;
    return;
  }
  const sha_words b0 = xmd_b0(msgs + lo, hi - lo, 48u * count, dp);
  const sha_words b1 = xmd_bi(b0, b0, 1, dp);
  const sha_words b2 = xmd_bi(b0, b1, 2, dp);
  // u_0 = OS2IP(uniform_bytes[0 .. 48)) mod p: the top 16 bytes are b_1's words 0..3, the low 32 its words 4..7 and b_2's 0..3
  uint32_t hw[8], lw[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hw[k] = b1.w[3 - k];
    hw[4 + k] = 0;
    lw[k] = b2.w[3 - k];
    lw[4 + k] = b1.w[7 - k];
  }
  pt29 acc = h2c_map_to_curve(h2c_wide_reduce(hw, lw));
  if (count == 2) {
    // u_1 from uniform_bytes[48 .. 96): b_2's words 4..7, then b_3
    const sha_words b3 = xmd_bi(b0, b2, 3, dp);
#pragma unroll
    for (int k = 0; k < 4; ++k) hw[k] = b2.w[7 - k];
#pragma unroll
    for (int k = 0; k < 8; ++k) lw[k] = b3.w[7 - k];
    acc = pt29_add(acc, h2c_map_to_curve(h2c_wide_reduce(hw, lw)));            // Q0 + Q1, complete: a doubling or the identity included
  }
  h2c_store(rec, acc);
}

// message bytes -> len_in_bytes uniform bytes (1 .. 8160: ell <= 255)
__global__ void __launch_bounds__(256)
k_h2c_expand(uint32_t n, uint32_t len_in_bytes, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint64_t msg_len,
             uint64_t total, const h2c_dstp* __restrict__ dp, uint8_t* __restrict__ out, uint32_t* __restrict__ status) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  uint8_t* o = out + idx * (size_t)len_in_bytes;
  uint64_t lo, hi;
  if (!h2c_msg_range(lo, hi, idx, offs, msg_len, total)) {
    atomicOr(status, 1u);
    for (uint32_t i = 0; i < len_in_bytes; ++i) o[i] = 0;
    return;
  }
  const sha_words b0 = xmd_b0(msgs + lo, hi - lo, len_in_bytes, dp);
  sha_words b = b0;
  const uint32_t ell = (len_in_bytes + 31) / 32;
#pragma unroll 1
  for (uint32_t i = 1; i <= ell; ++i) {
    b = xmd_bi(b0, b, i, dp);
    const uint32_t at = (i - 1) * 32, take = len_in_bytes - at < 32 ? len_in_bytes - at : 32;
#pragma unroll
    for (int k = 0; k < 32; ++k)
      if ((uint32_t)k < take) o[at + k] = (uint8_t)(b.w[k >> 2] >> (24 - 8 * (k & 3)));
  }
}

// uniform bytes -> record: out[i] = sum over j < count of map_to_curve(OS2IP(uniform[(i count + j) len ...]) mod p), 32 <= len <= 64
__global__ void __launch_bounds__(256)
k_h2c_map(uint32_t n, uint32_t count, uint32_t len, const uint8_t* __restrict__ uniform, uint8_t* __restrict__ out) {
  size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const uint32_t hi_len = len - 32;     // 0 .. 32 bytes above the low 256 bits
  pt29 acc = pt29_identity();
#pragma unroll 1
  for (uint32_t j = 0; j < count; ++j) {
    const uint8_t* p = uniform + (idx * count + j) * (size_t)len;
    uint32_t hw[8], lw[8];
    load_be32_unaligned(lw, p + hi_len);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t from_end = (uint32_t)(4 * k + b);        // byte of weight 256^from_end
        if (from_end < hi_len) word |= (uint32_t)p[hi_len - 1 - from_end] << (8 * b);
      }
      hw[k] = word;
    }
    const pt29 q = h2c_map_to_curve(h2c_wide_reduce(hw, lw));
    acc = j == 0 ? q : pt29_add(acc, q);
  }
  h2c_store(out + idx * 65, acc);
}

// the context's block for this file: status word and DST_prime on the device, the pinned block both travel through
int h2c_block(s2k_ctx* ctx) {
  if (!ctx->h2c_dev) HIP_TRY(ctx, hipMalloc(&ctx->h2c_dev, H2C_BLOCK_BYTES));
  if (!ctx->h2c_host) HIP_TRY(ctx, hipHostMalloc(&ctx->h2c_host, H2C_BLOCK_BYTES, hipHostMallocDefault));
  return S2K_OK;
}

const char* h2c_offsets_check(size_t n, const uint64_t* off) {
  if (off[0] != 0) return "msg_offsets must start at 0";
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return "msg_offsets must not decrease";
  return nullptr;
}

// Enqueue one expansion or hash on `st` (device pointers), synchronise, read the status word.  len_in_bytes == 0: records
// of `count` mapped points (k_h2c_hash); else uniform bytes (k_h2c_expand).  The host forms pass h_msgs / h_offs: copied to
// d_msgs / d_offs (the context's staging block) on `st` AFTER ctx_enter, so that the copies too queue behind a *_device
// call of this context that is still in flight on another stream and may be using that block.
int h2c_run(s2k_ctx* ctx, hipStream_t st, size_t n, const h2c_dstp& dstp, const void* d_msgs, const void* d_offs, size_t msg_len,
            size_t total, uint32_t count, uint32_t len_in_bytes, void* d_out, const uint8_t* h_msgs = nullptr,
            const uint64_t* h_offs = nullptr) {
  int rc = h2c_block(ctx);
  if (rc) return rc;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  if (h_msgs && total) HIP_TRY(ctx, hipMemcpyAsync((void*)d_msgs, h_msgs, total, hipMemcpyHostToDevice, st));
  if (h_offs) HIP_TRY(ctx, hipMemcpyAsync((void*)d_offs, h_offs, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  uint8_t* h = (uint8_t*)ctx->h2c_host;
  uint8_t* d = (uint8_t*)ctx->h2c_dev;
  // (every call of this file ends with a synchronisation of its stream, so the pinned block is free again here)
  memset(h, 0, H2C_DSTP_OFF);
  memcpy(h + H2C_DSTP_OFF, &dstp, sizeof dstp);
  HIP_TRY(ctx, hipMemcpyAsync(d, h, H2C_DSTP_OFF + sizeof dstp, hipMemcpyHostToDevice, st));
  uint32_t* d_status = (uint32_t*)d;
  const h2c_dstp* d_dstp = (const h2c_dstp*)(d + H2C_DSTP_OFF);
  if (len_in_bytes)
    k_h2c_expand<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, len_in_bytes, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, (uint64_t)msg_len,
                                                 (uint64_t)total, d_dstp, (uint8_t*)d_out, d_status);
  else
    k_h2c_hash<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, count, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, (uint64_t)msg_len,
                                               (uint64_t)total, d_dstp, (uint8_t*)d_out, d_status);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(h, d, 4, hipMemcpyDeviceToHost, st));
  rc = ctx_leave(ctx, st);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;   // the stream has been synchronised: nothing of this context is in flight
  uint32_t h_status;
  memcpy(&h_status, h, 4);
  if (h_status) return fail(ctx, S2K_ERR_ARG, "message offsets decrease or leave the message buffer");
  return S2K_OK;
}

// the checks the host forms of the message entry points share; *total receives the message bytes
int h2c_check_msgs(s2k_ctx* ctx, size_t n, const uint8_t* dst, size_t dst_len, const uint8_t* msgs, const uint64_t* msg_offsets,
                   size_t msg_len, const void* out, h2c_dstp* dstp, size_t* total) {
  if (!dst || dst_len == 0) return fail(ctx, S2K_ERR_ARG, "empty domain separation tag");
  dstp->len = (uint32_t)s2k_h2c::dst_prime(dst, dst_len, dstp->b);
  if (n == 0) return S2K_OK;
  if (n > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  if (!out) return fail(ctx, S2K_ERR_ARG, "null output buffer");
  if (msg_offsets) {
    if (const char* e = h2c_offsets_check(n, msg_offsets)) return fail(ctx, S2K_ERR_ARG, "%s", e);
    *total = (size_t)msg_offsets[n];
  } else {
    if (msg_len && n > SIZE_MAX / msg_len) return fail(ctx, S2K_ERR_ARG, "message buffer too large");
    *total = n * msg_len;
  }
  if (*total && !msgs) return fail(ctx, S2K_ERR_ARG, "null message buffer");
  return S2K_OK;
}

// host buffers: stage messages and offsets, run, copy `out_bytes` back
int h2c_host_call(s2k_ctx* ctx, size_t n, const h2c_dstp& dstp, const uint8_t* msgs, const uint64_t* msg_offsets, size_t msg_len, size_t total,
                  uint32_t count, uint32_t len_in_bytes, uint8_t* out, size_t out_bytes) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  const size_t sizes[3] = {total + 16, (n + 1) * sizeof(uint64_t), out_bytes + 16};
  uint8_t* d[3];
  rc = ctx_stage(ctx, sizes, 3, d);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  rc = h2c_run(ctx, st, n, dstp, d[0], msg_offsets ? d[1] : nullptr, msg_len, total, count, len_in_bytes, d[2], msgs, msg_offsets);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpy(out, d[2], out_bytes, hipMemcpyDeviceToHost));
  return S2K_OK;
}

}  // namespace

extern "C" {

int s2k_h2c_dst_prime(const uint8_t* dst, size_t dst_len, uint8_t out[256], size_t* out_len) {
  if (!dst || !out || !out_len || dst_len == 0) return S2K_ERR_ARG;
  *out_len = s2k_h2c::dst_prime(dst, dst_len, out);
  return S2K_OK;
}

int s2k_expand_message_xmd_batch(s2k_ctx* ctx, size_t n, const uint8_t* dst, size_t dst_len, const uint8_t* msgs,
                                 const uint64_t* msg_offsets, size_t msg_len, size_t len_in_bytes, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (len_in_bytes < 1 || len_in_bytes > 8160) return fail(ctx, S2K_ERR_ARG, "len_in_bytes must be in 1..8160");
  h2c_dstp dstp{};
  size_t total = 0;
  int rc = h2c_check_msgs(ctx, n, dst, dst_len, msgs, msg_offsets, msg_len, out, &dstp, &total);
  if (rc || n == 0) return rc;
  return h2c_host_call(ctx, n, dstp, msgs, msg_offsets, msg_len, total, 0, (uint32_t)len_in_bytes, out, n * len_in_bytes);
}

int s2k_hash_to_curve_batch(s2k_ctx* ctx, int suite, size_t n, const uint8_t* dst, size_t dst_len, const uint8_t* msgs,
                            const uint64_t* msg_offsets, size_t msg_len, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (suite != S2K_H2C_SSWU_RO && suite != S2K_H2C_SSWU_NU) return fail(ctx, S2K_ERR_ARG, "unknown suite");
  h2c_dstp dstp{};
  size_t total = 0;
  int rc = h2c_check_msgs(ctx, n, dst, dst_len, msgs, msg_offsets, msg_len, out, &dstp, &total);
  if (rc || n == 0) return rc;
  return h2c_host_call(ctx, n, dstp, msgs, msg_offsets, msg_len, total, suite == S2K_H2C_SSWU_RO ? 2 : 1, 0, out, n * 65);
}

int s2k_hash_to_curve_batch_device(s2k_ctx* ctx, int suite, size_t n, const uint8_t* dst, size_t dst_len, const void* d_msgs,
                                   const void* d_msg_offsets, size_t msg_len, size_t total_msg_bytes, void* d_out, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (suite != S2K_H2C_SSWU_RO && suite != S2K_H2C_SSWU_NU) return fail(ctx, S2K_ERR_ARG, "unknown suite");
  if (!dst || dst_len == 0) return fail(ctx, S2K_ERR_ARG, "empty domain separation tag");
  if (n == 0) return S2K_OK;
  if (n > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  if (!d_out) return fail(ctx, S2K_ERR_ARG, "null output buffer");
  if (total_msg_bytes && !d_msgs) return fail(ctx, S2K_ERR_ARG, "null message buffer");
  if (!d_msg_offsets && msg_len && (n > SIZE_MAX / msg_len || n * msg_len > total_msg_bytes))
    return fail(ctx, S2K_ERR_ARG, "n * msg_len exceeds total_msg_bytes");
  h2c_dstp dstp{};
  dstp.len = (uint32_t)s2k_h2c::dst_prime(dst, dst_len, dstp.b);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return h2c_run(ctx, (hipStream_t)hip_stream, n, dstp, d_msgs, d_msg_offsets, msg_len, total_msg_bytes,
                 suite == S2K_H2C_SSWU_RO ? 2 : 1, 0, d_out);
}

int s2k_map_to_curve_batch(s2k_ctx* ctx, size_t n, size_t count, size_t len, const uint8_t* uniform, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (count != 1 && count != 2) return fail(ctx, S2K_ERR_ARG, "count must be 1 or 2");
  if (len < 32 || len > 64) return fail(ctx, S2K_ERR_ARG, "len must be in 32..64");   // (SetWideBytes panics, field_reduce.go:39,62)
  if (n == 0) return S2K_OK;
  if (n > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large");
  if (!uniform || !out) return fail(ctx, S2K_ERR_ARG, "null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  const size_t in_bytes = n * count * len, sizes[2] = {in_bytes + 16, n * 65 + 16};
  uint8_t* d[2];
  rc = ctx_stage(ctx, sizes, 2, d);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(d[0], uniform, in_bytes, hipMemcpyHostToDevice, st));
  k_h2c_map<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, (uint32_t)count, (uint32_t)len, d[0], d[1]);
  HIP_TRY(ctx, hipGetLastError());
  rc = ctx_leave(ctx, st);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemcpyAsync(out, d[1], n * 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  return S2K_OK;
}

}  // extern "C"
