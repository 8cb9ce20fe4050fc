// h2c_host.h — the host half of hashing to the curve: a small SHA-256 (FIPS 180-4) and DST_prime of expand_message_xmd
// (RFC 9380 5.3.1 / 5.3.3; the reference's h2c_expand_message.go:46-63).  Plain C++, no HIP: h2c.hip uses it before it
// launches, and tests/c/h2c_sanitize_main.cpp builds it host-only under AddressSanitizer + UBSan, because both functions
// take caller-supplied lengths.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace s2k_h2c {

struct sha256 {
  uint32_t st[8];
  uint8_t buf[64];
  uint64_t len;   // bytes taken so far

  sha256() { reset(); }
  void reset() {
    static const uint32_t iv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    memcpy(st, iv, sizeof st);
    len = 0;
  }
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const uint8_t* p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u,
        0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu,
        0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u,
        0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
        0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u,
        0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u,
        0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
  }
  void update(const uint8_t* p, size_t n) {
    size_t have = (size_t)(len & 63);
    len += n;
    if (have) {
      size_t take = 64 - have < n ? 64 - have : n;
      memcpy(buf + have, p, take);
      p += take;
      n -= take;
      if (have + take < 64) return;
      block(buf);
    }
    for (; n >= 64; p += 64, n -= 64) block(p);
    if (n) memcpy(buf, p, n);
  }
  void final(uint8_t out[32]) {
    const uint64_t bits = len * 8;
    size_t have = (size_t)(len & 63);
    buf[have++] = 0x80;
    if (have > 56) {
      memset(buf + have, 0, 64 - have);
      block(buf);
      have = 0;
    }
    memset(buf + have, 0, 56 - have);
    for (int i = 0; i < 8; ++i) buf[56 + i] = (uint8_t)(bits >> (56 - 8 * i));
    block(buf);
    for (int i = 0; i < 8; ++i) {
      out[4 * i] = (uint8_t)(st[i] >> 24);
      out[4 * i + 1] = (uint8_t)(st[i] >> 16);
      out[4 * i + 2] = (uint8_t)(st[i] >> 8);
      out[4 * i + 3] = (uint8_t)st[i];
    }
  }
};

// DST_prime = DST || I2OSP(len(DST), 1), a tag of more than 255 bytes hashed first (h2c_expand_message.go:54-63).
// out holds 256 bytes; returns the length written, or 0 for an empty tag (which the reference refuses, :50-53).
inline size_t dst_prime(const uint8_t* dst, size_t dst_len, uint8_t out[256]) {
  if (!dst || dst_len == 0) return 0;
  if (dst_len > 255) {
    static const char tag[] = "H2C-OVERSIZE-DST-";
    sha256 h;
    h.update((const uint8_t*)tag, sizeof tag - 1);
    h.update(dst, dst_len);
    h.final(out);
    out[32] = 32;
    return 33;
  }
  memcpy(out, dst, dst_len);
  out[dst_len] = (uint8_t)dst_len;
  return dst_len + 1;
}

}  // namespace s2k_h2c
