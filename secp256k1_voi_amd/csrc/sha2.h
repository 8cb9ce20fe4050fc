// sha2.h — SHA-256 and SHA-512 (FIPS 180-4) over (bytes, len), one message per caller: the hash cores of the message
// digests (digest.hip: k_digest_messages hashes one message per lane).  Under hipcc this is DEVICE code only: the functions are
// marked __host__ __device__ so that they compile, but the round constants are __constant__, whose host shadow is never
// filled, and a host call returns a wrong digest (sha256_hash("abc") gives the initial state 6a09e667...5be0cd19 at -O3) - the
// library's host code has a SHA-256 of its own (rlc.hip).  It RUNS on the host only as plain C++ (no HIP header is needed then),
// the way der.h and h2c_host.h do: tests/c/sha2_sanitize_main.cpp builds it so under AddressSanitizer + UBSan, because both
// drivers take a caller-supplied length.  sha256.h (the BIP-340 challenge) is left as it is; the compression here is the same 16-word
// rolling schedule under a name of its own.
//
// Lengths are below 2^31 bytes.  A driver reads msg[0 .. len) and nothing else: the padding (0x80, zeros, the bit length in
// the last 8 or 16 bytes of the last block) is made in registers, never read.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define S2K_SHA2_FN __host__ __device__ __forceinline__
#define S2K_SHA2_TABLE __constant__ const
#else
#define S2K_SHA2_FN inline
#define S2K_SHA2_TABLE static const
#endif

namespace s2k_sha2 {

// (read with compile-time indices from fully unrolled rounds, uniformly over the wave: scalar loads or literals, no VGPR)
S2K_SHA2_TABLE uint32_t K256[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
    0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
    0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
    0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
    0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
    0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
S2K_SHA2_TABLE uint64_t K512[80] = {
    0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
    0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
    0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
    0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
    0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
    0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
    0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
    0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
    0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
    0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
    0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
    0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
    0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
    0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};

// v_alignbit_b32: the low 32 bits of (hi:lo) >> n, n in [0, 31]
S2K_SHA2_FN uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t n) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_alignbit(hi, lo, n);
#else
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (n & 31u));
#endif
}
S2K_SHA2_FN uint32_t rotr32(uint32_t x, uint32_t n) { return alignbit(x, x, n); }
// a 64-bit rotate is two alignbits on the halves; by 32 or more the halves trade places first, which costs nothing
template <int N>
S2K_SHA2_FN uint64_t rotr64(uint64_t x) {
  static_assert(N > 0 && N < 64, "rotate count");
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  const uint32_t a = N < 32 ? lo : hi, b = N < 32 ? hi : lo;      // the rotated word is (b:a) >> (N mod 32), cyclically
  constexpr uint32_t m = (uint32_t)(N & 31);
  const uint32_t rl = m ? alignbit(b, a, m) : a, rh = m ? alignbit(a, b, m) : b;
  return ((uint64_t)rh << 32) | rl;
}

// one 64-byte block, w = 16 big-endian words; 16-word rolling schedule (the model: sha256_compress of sha256.h)
S2K_SHA2_FN void sha256_compress(uint32_t st[8], uint32_t w[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    uint32_t wi;
    if (i < 16) {
      wi = w[i];
    } else {
      const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
      const uint32_t s0 = rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10);
      wi = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
      w[i & 15] = wi;
    }
    const uint32_t S1 = rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = h + S1 + ch + K256[i] + wi;
    const uint32_t S0 = rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22);
    const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + mj;
    h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// one 128-byte block, w = 16 big-endian 64-bit words: the same rolling schedule, 16 x 64 bits = 32 registers.  Sixteen rounds
// are unrolled, so every index into w is a constant, and rounds 16..79 are four turns of a loop over them: K512 is then read
// from constant memory at a uniform, running index (scalar loads), and the 64 live registers - the words, the state, its copy
// for the final addition - stay 64.  (All 80 rounds unrolled, the compiler rolled them up again less tidily: 113 registers for
// the compression alone, and the digest kernel, held to 128 for four waves per SIMD, spilled.)
S2K_SHA2_FN void sha512_round(uint64_t& a, uint64_t& b, uint64_t& c, uint64_t& d, uint64_t& e, uint64_t& f, uint64_t& g, uint64_t& h,
                              uint64_t k, uint64_t wi) {
  const uint64_t S1 = rotr64<14>(e) ^ rotr64<18>(e) ^ rotr64<41>(e);
  const uint64_t ch = (e & f) ^ (~e & g);
  const uint64_t t1 = h + S1 + ch + k + wi;
  const uint64_t S0 = rotr64<28>(a) ^ rotr64<34>(a) ^ rotr64<39>(a);
  const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
  const uint64_t t2 = S0 + mj;
  h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
}
S2K_SHA2_FN void sha512_compress(uint64_t st[8], uint64_t w[16]) {
  uint64_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
  for (int j = 0; j < 16; ++j) sha512_round(a, b, c, d, e, f, g, h, K512[j], w[j]);
#pragma unroll 1
  for (int t = 16; t < 80; t += 16) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint64_t w15 = w[(j + 1) & 15], w2 = w[(j + 14) & 15];
      const uint64_t s0 = rotr64<1>(w15) ^ rotr64<8>(w15) ^ (w15 >> 7);
      const uint64_t s1 = rotr64<19>(w2) ^ rotr64<61>(w2) ^ (w2 >> 6);
      w[j] += s0 + w[(j + 9) & 15] + s1;
      sha512_round(a, b, c, d, e, f, g, h, K512[t + j], w[j]);
    }
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// the 4 bytes at pos of the padded message, as one big-endian word: message bytes below len, 0x80 at len, zeros behind it
// (the length field is put in by the drivers)
S2K_SHA2_FN uint32_t padded_word(const uint8_t* msg, uint32_t len, uint32_t pos) {
  if (pos + 4 <= len) return ((uint32_t)msg[pos] << 24) | ((uint32_t)msg[pos + 1] << 16) | ((uint32_t)msg[pos + 2] << 8) | msg[pos + 3];
  uint32_t word = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t p = pos + j;
    const uint32_t byte = p < len ? msg[p] : (p == len ? 0x80u : 0u);
    word = (word << 8) | byte;
  }
  return word;
}

S2K_SHA2_FN void sha256_init(uint32_t st[8]) {
  st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
  st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}
S2K_SHA2_FN void sha512_init(uint64_t st[8]) {
  st[0] = 0x6a09e667f3bcc908ull; st[1] = 0xbb67ae8584caa73bull; st[2] = 0x3c6ef372fe94f82bull; st[3] = 0xa54ff53a5f1d36f1ull;
  st[4] = 0x510e527fade682d1ull; st[5] = 0x9b05688c2b3e6c1full; st[6] = 0x1f83d9abfb41bd6bull; st[7] = 0x5be0cd19137e2179ull;
}

// blocks of the padded message: len bytes, the 0x80 and the length field
S2K_SHA2_FN uint32_t sha256_blocks(uint32_t len) { return (len + 9 + 63) / 64; }
S2K_SHA2_FN uint32_t sha512_blocks(uint32_t len) { return (len + 17 + 127) / 128; }

// st = the hash state after every block of the padded message of len bytes.  In a kernel each lane runs the block count of
// its own message: the wave runs to the longest of them, the lanes that are done masked off.
S2K_SHA2_FN void sha256_message(uint32_t st[8], const uint8_t* msg, uint32_t len) {
  sha256_init(st);
  const uint32_t nblocks = sha256_blocks(len);
#pragma unroll 1
  for (uint32_t blk = 0; blk < nblocks; ++blk) {
    uint32_t w[16];
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i) w[i] = padded_word(msg, len, blk * 64 + i * 4);
    if (blk == nblocks - 1) {
      w[14] = len >> 29;                                   // the bit length, 64 bits big-endian (len < 2^31)
      w[15] = len << 3;
    }
    sha256_compress(st, w);
  }
}
S2K_SHA2_FN void sha512_message(uint64_t st[8], const uint8_t* msg, uint32_t len) {
  sha512_init(st);
  const uint32_t nblocks = sha512_blocks(len);
#pragma unroll 1
  for (uint32_t blk = 0; blk < nblocks; ++blk) {
    uint64_t w[16];
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
      w[i] = ((uint64_t)padded_word(msg, len, blk * 128 + i * 8) << 32) | padded_word(msg, len, blk * 128 + i * 8 + 4);
    if (blk == nblocks - 1) {
      w[14] = 0;                                           // the bit length, 128 bits big-endian
      w[15] = (uint64_t)len << 3;
    }
    sha512_compress(st, w);
  }
}
// SHA-256 of the 32-byte digest in st (its 8 big-endian words), into st: the second half of Bitcoin's double SHA-256
S2K_SHA2_FN void sha256_again(uint32_t st[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = st[i];
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; ++i) w[i] = 0;
  w[15] = 256;
  sha256_init(st);
  sha256_compress(st, w);
}

// byte-string forms (the host program; the kernel stores the state words itself)
S2K_SHA2_FN void sha256_hash(const uint8_t* msg, uint32_t len, uint8_t out[32], bool twice = false) {
  uint32_t st[8];
  sha256_message(st, msg, len);
  if (twice) sha256_again(st);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(st[i] >> (24 - 8 * j));
}
S2K_SHA2_FN void sha512_hash(const uint8_t* msg, uint32_t len, uint8_t out[64]) {
  uint64_t st[8];
  sha512_message(st, msg, len);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(st[i] >> (56 - 8 * j));
}

}  // namespace s2k_sha2
