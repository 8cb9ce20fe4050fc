// The Keccak cores (csrc/keccak.h: Keccak-256 and SHA3-256 over a caller-supplied length, and the fixed 64-byte case of the
// addresses) in their host build, under AddressSanitizer + UBSan.  Every message lives in a heap buffer of its exact length,
// so one byte read past the end is a report; digests go to exact-size heap buffers too.  The program prints one line per
// digest and judges nothing itself: tests/test_keccak_sanitize_cpu.py compares every line with hashlib and the model.
//   vec <index> <keccak256> <sha3_256>     the empty string, "abc", and Gx || Gy (the key of secret 1)
//   len <length> <keccak256> <sha3_256>    every length 0..300, byte i of the message of length n = (131 i + 7 n + 1) mod 256
//   xy <index> <keccak256_64> <keccak256>  16 patterned 64-byte inputs: the single-block case and the general driver
// Built host-only (g++ -fsanitize=address,undefined) and run on the CPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "keccak.h"

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}

static const uint8_t GXY[64] = {
    0x79, 0xBE, 0x66, 0x7E, 0xF9, 0xDC, 0xBB, 0xAC, 0x55, 0xA0, 0x62, 0x95, 0xCE, 0x87, 0x0B, 0x07, 0x02, 0x9B, 0xFC, 0xDB, 0x2D, 0xCE,
    0x28, 0xD9, 0x59, 0xF2, 0x81, 0x5B, 0x16, 0xF8, 0x17, 0x98, 0x48, 0x3A, 0xDA, 0x77, 0x26, 0xA3, 0xC4, 0x65, 0x5D, 0xA4, 0xFB, 0xFC,
    0x0E, 0x11, 0x08, 0xA8, 0xFD, 0x17, 0xB4, 0x48, 0xA6, 0x85, 0x54, 0x19, 0x9C, 0x47, 0xD0, 0x8F, 0xFB, 0x10, 0xD4, 0xB8};

static void line(const char* kind, unsigned tag, const uint8_t* p, size_t n) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);             // exact size (malloc(0) may return null): overreads trip ASan
  if (n) memcpy(in, p, n);
  const uint8_t* msg = n ? in : in + 1;                   // length 0: a pointer with NO readable byte behind it
  uint8_t *k = (uint8_t*)malloc(32), *s3 = (uint8_t*)malloc(32);
  s2k_keccak::keccak256_hash(msg, (uint32_t)n, s2k_keccak::DOMAIN_KECCAK, k);
  s2k_keccak::keccak256_hash(msg, (uint32_t)n, s2k_keccak::DOMAIN_SHA3, s3);
  printf("%s %u %s %s\n", kind, tag, hex(k, 32).c_str(), hex(s3, 32).c_str());
  free(s3);
  free(k);
  free(in);
}

int main() {
  line("vec", 0, (const uint8_t*)"", 0);
  line("vec", 1, (const uint8_t*)"abc", 3);
  line("vec", 2, GXY, 64);
  for (unsigned n = 0; n <= 300; ++n) {
    uint8_t buf[300];
    for (unsigned i = 0; i < n; ++i) buf[i] = (uint8_t)(131u * i + 7u * n + 1u);
    line("len", n, buf, n);
  }
  for (unsigned t = 0; t < 16; ++t) {
    uint8_t* xy = (uint8_t*)malloc(64);
    for (unsigned i = 0; i < 64; ++i) xy[i] = t == 0 ? 0 : (t == 1 ? 0xff : (uint8_t)(29u * i + 83u * t + (i >> 3) * t));
    uint64_t d[4];
    s2k_keccak::keccak256_64(d, xy);
    uint8_t one[32], gen[32];
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 8; ++j) one[8 * i + j] = (uint8_t)(d[i] >> (8 * j));
    s2k_keccak::keccak256_hash(xy, 64, s2k_keccak::DOMAIN_KECCAK, gen);
    printf("xy %u %s %s\n", t, hex(one, 32).c_str(), hex(gen, 32).c_str());
    free(xy);
  }
  printf("done\n");
  return 0;
}
