// keccak.h — Keccak-f[1600] and the two 256-bit sponges over it, one message per caller: Keccak-256 (the original padding,
// domain byte 0x01: the hash of Ethereum's addresses and message digests) and SHA3-256 (FIPS 202, domain byte 0x06).  The
// hash cores of k_digest_keccak (digest.hip: one message per lane) and k_keccak_address (address.hip: one key record per
// lane).  As sha2.h: under hipcc it is device code only (the round constants are __constant__; a host call there returns a
// wrong digest), and it runs on the host only as plain C++ (tests/c/keccak_sanitize_main.cpp builds it so under
// AddressSanitizer + UBSan, because the driver takes a caller-supplied length).
//
// The state is 25 lanes of 64 bits, a[x + 5 y].  Every index into it is a compile-time constant, so on the device it is 50
// registers and never memory; a round produces the next state row by row (keccak_row), so that little more than one state
// is live at a time.  The 24 rounds are a rolled loop whose only running index reads the round constant, uniformly over the
// wave (a scalar load).
//
// Lengths are below 2^31 bytes.  A driver reads msg[0 .. len) and nothing else: the padding (the domain byte at len, zeros,
// 0x80 in the last byte of the last block) is made in registers, never read.
#pragma once
#include <stdint.h>

#include "sha2.h"   // rotr64<N>: two v_alignbit_b32, the halves trade places for free at 32 and above

#if defined(__HIPCC__)
#define S2K_KECCAK_FN __host__ __device__ __forceinline__
#define S2K_KECCAK_TABLE __constant__ const
#else
#define S2K_KECCAK_FN inline
#define S2K_KECCAK_TABLE static const
#endif

namespace s2k_keccak {

constexpr uint32_t RATE = 136;            // bytes a block absorbs: 1600 / 8 - 2 * 32
constexpr uint8_t DOMAIN_KECCAK = 0x01;   // Keccak-256 as submitted
constexpr uint8_t DOMAIN_SHA3 = 0x06;     // FIPS 202 SHA3-256

// iota's constants (FIPS 202, 3.2.5; tests/keccak_model.py generates the same 24 from the LFSR)
S2K_KECCAK_TABLE uint64_t RC[24] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
    0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// rho's rotation of lane (x, y): (t + 1)(t + 2) / 2 along the walk (x, y) -> (y, 2x + 3y) from (1, 0); lane (0, 0) stays
constexpr int rho_of(int x, int y) {
  int cx = 1, cy = 0;
  for (int t = 0; t < 24; ++t) {
    if (cx == x && cy == y) return ((t + 1) * (t + 2) / 2) % 64;
    const int nx = cy, ny = (2 * cx + 3 * cy) % 5;
    cx = nx;
    cy = ny;
  }
  return 0;
}
static_assert(rho_of(0, 0) == 0 && rho_of(1, 0) == 1 && rho_of(2, 0) == 62 && rho_of(0, 1) == 36 && rho_of(0, 2) == 3 && rho_of(3, 3) == 21 &&
                  rho_of(4, 4) == 14 && rho_of(1, 1) == 44,
              "rho offsets");

template <int N>
S2K_KECCAK_FN uint64_t rotl64(uint64_t x) {
  if constexpr (N == 0)
    return x;
  else
    return s2k_sha2::rotr64<64 - N>(x);
}

// Lane (X, Y) of the state behind theta, rho and pi.  pi moves lane (x, y) to (y, 2x + 3y), so what arrives at (X, Y) left
// from x = X + 3Y, y = X; theta's column term d[x] is folded in here, so no lane is written twice in a round.
template <int X, int Y>
S2K_KECCAK_FN uint64_t theta_rho_pi(const uint64_t (&a)[25], const uint64_t (&d)[5]) {
  constexpr int x = (X + 3 * Y) % 5, y = X;
  return rotl64<rho_of(x, y)>(a[x + 5 * y] ^ d[x]);
}
// Row Y of the next state: chi over the five lanes that arrive in it.  A round is five of these: each reads five lanes of the
// old state for the last time and writes five of the new one, so about one state and a row are live at once, not two states.
template <int Y>
S2K_KECCAK_FN void keccak_row(uint64_t (&e)[25], const uint64_t (&a)[25], const uint64_t (&d)[5]) {
  const uint64_t b[5] = {theta_rho_pi<0, Y>(a, d), theta_rho_pi<1, Y>(a, d), theta_rho_pi<2, Y>(a, d), theta_rho_pi<3, Y>(a, d),
                         theta_rho_pi<4, Y>(a, d)};
#pragma unroll
  for (int x = 0; x < 5; ++x) e[x + 5 * Y] = b[x] ^ (~b[(x + 1) % 5] & b[(x + 2) % 5]);
}

S2K_KECCAK_FN void keccak_round(uint64_t (&a)[25], uint64_t rc) {
  uint64_t c[5], d[5], e[25];
#pragma unroll
  for (int x = 0; x < 5; ++x) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];          // theta: column parities
#pragma unroll
  for (int x = 0; x < 5; ++x) d[x] = c[(x + 4) % 5] ^ rotl64<1>(c[(x + 1) % 5]);
  keccak_row<0>(e, a, d);
  keccak_row<1>(e, a, d);
  keccak_row<2>(e, a, d);
  keccak_row<3>(e, a, d);
  keccak_row<4>(e, a, d);
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = e[i];
  a[0] ^= rc;                                                                                        // iota
}

S2K_KECCAK_FN void keccak_f1600(uint64_t (&a)[25]) {
#pragma unroll 1
  for (int r = 0; r < 24; ++r) keccak_round(a, RC[r]);
}

// eight message bytes as one little-endian lane (any alignment: bytes)
S2K_KECCAK_FN uint64_t load_lane(const uint8_t* p) {
  uint64_t lane = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8; ++j) lane |= (uint64_t)p[j] << (8 * j);
  return lane;
}

// blocks of the padded message: the domain byte always follows the message, so a message of a whole number of blocks has one more
S2K_KECCAK_FN uint32_t keccak256_blocks(uint32_t len) { return len / RATE + 1; }

// out4 = the first four lanes of the state after every block of the padded message: the digest, little-endian lane by lane.
// Every block but the last is 17 whole lanes of the message.  The last holds rem = len mod 136 bytes: rem / 8 whole lanes, then
// ONE lane with the remaining bytes and the domain byte behind them, then zeros, and 0x80 on top of byte 135 - so only that
// one lane is put together byte by byte under a condition.  In a kernel each lane of the wave runs the block count of its
// own message, the lanes that are done masked off.
S2K_KECCAK_FN void keccak256_message(uint64_t out4[4], const uint8_t* msg, uint32_t len, uint8_t domain) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) a[i] = 0;
  const uint32_t nblocks = keccak256_blocks(len);
#pragma unroll 1
  for (uint32_t blk = 0; blk + 1 < nblocks; ++blk) {
#pragma unroll
    for (uint32_t i = 0; i < RATE / 8; ++i) a[i] ^= load_lane(msg + blk * RATE + i * 8);
    keccak_f1600(a);
  }
  const uint8_t* tail = msg + (nblocks - 1) * RATE;
  const uint32_t rem = len - (nblocks - 1) * RATE, whole = rem >> 3;     // rem <= 135: whole <= 16
  uint64_t part = (uint64_t)domain << (8 * (rem & 7u));
#pragma unroll
  for (uint32_t j = 0; j < 7; ++j)
    if (whole * 8 + j < rem) part |= (uint64_t)tail[whole * 8 + j] << (8 * j);
#pragma unroll
  for (uint32_t i = 0; i < RATE / 8; ++i) {
    if (i < whole) a[i] ^= load_lane(tail + i * 8);
    a[i] ^= i == whole ? part : 0;
  }
  a[RATE / 8 - 1] ^= 0x80ull << 56;                         // byte 135; on top of the domain byte there: 0x81 / 0x86
  keccak_f1600(a);
#pragma unroll
  for (int i = 0; i < 4; ++i) out4[i] = a[i];
}

// Keccak-256 of exactly 64 bytes (X || Y of a public key), one block: the address is bytes 12..32 of the digest
S2K_KECCAK_FN void keccak256_64(uint64_t out4[4], const uint8_t xy[64]) {
  uint64_t a[25];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t lane = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) lane |= (uint64_t)xy[8 * i + j] << (8 * j);
    a[i] = lane;
  }
#pragma unroll
  for (int i = 8; i < 25; ++i) a[i] = 0;
  a[8] ^= DOMAIN_KECCAK;
  a[16] ^= 0x80ull << 56;
  keccak_f1600(a);
#pragma unroll
  for (int i = 0; i < 4; ++i) out4[i] = a[i];
}

// byte-string form (the host program; the kernels store the lanes themselves)
S2K_KECCAK_FN void keccak256_hash(const uint8_t* msg, uint32_t len, uint8_t domain, uint8_t out[32]) {
  uint64_t d[4];
  keccak256_message(d, msg, len, domain);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) out[8 * i + j] = (uint8_t)(d[i] >> (8 * j));
}

}  // namespace s2k_keccak
