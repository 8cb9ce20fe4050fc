// The hash cores of the message digests (csrc/sha2.h: SHA-256, double SHA-256 and SHA-512 over a caller-supplied length) in
// their host build, under AddressSanitizer + UBSan.  Every message lives in a heap buffer of its exact length, so one byte
// read past the end is a report; digests go to exact-size heap buffers too.  The program prints one line per digest and
// judges nothing itself: tests/test_sha2_sanitize_cpu.py compares every line with hashlib.
//   fips <index> <sha256> <sha256d> <sha512>     the FIPS 180-4 example messages below
//   len <length> <sha256> <sha256d> <sha512>     every length 0..300, byte i of the message of length n = (131 i + 7 n + 1) mod 256
// Built host-only (g++ -fsanitize=address,undefined) and run on the CPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sha2.h"

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}

// FIPS 180-4 examples: "abc", the empty string, the 448-bit message (two SHA-256 blocks) and the 896-bit one (two SHA-512 blocks)
static const char* const FIPS[4] = {
    "abc", "", "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
    "abcdefghbcdefghicdefghijdefghijkefghijklfghijklmghijklmnhijklmnoijklmnopjklmnopqklmnopqrlmnopqrsmnopqrstnopqrstu"};

static void line(const char* kind, unsigned tag, const uint8_t* p, size_t n) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);             // exact size (malloc(0) may return null): overreads trip ASan
  if (n) memcpy(in, p, n);
  const uint8_t* msg = n ? in : in + 1;                   // length 0: a pointer with NO readable byte behind it
  uint8_t *o256 = (uint8_t*)malloc(32), *o256d = (uint8_t*)malloc(32), *o512 = (uint8_t*)malloc(64);
  s2k_sha2::sha256_hash(msg, (uint32_t)n, o256);
  s2k_sha2::sha256_hash(msg, (uint32_t)n, o256d, /*twice=*/true);
  s2k_sha2::sha512_hash(msg, (uint32_t)n, o512);
  printf("%s %u %s %s %s\n", kind, tag, hex(o256, 32).c_str(), hex(o256d, 32).c_str(), hex(o512, 64).c_str());
  free(o512);
  free(o256d);
  free(o256);
  free(in);
}

int main() {
  for (unsigned k = 0; k < 4; ++k) line("fips", k, (const uint8_t*)FIPS[k], strlen(FIPS[k]));
  for (unsigned n = 0; n <= 300; ++n) {
    uint8_t buf[300];
    for (unsigned i = 0; i < n; ++i) buf[i] = (uint8_t)(131u * i + 7u * n + 1u);
    line("len", n, buf, n);
  }
  // the rotates: alignbit's portable form against shifts, every count
  for (unsigned n = 1; n < 32; ++n) {
    const uint32_t x = 0x80c0e1f3u;
    if (s2k_sha2::rotr32(x, n) != ((x >> n) | (x << (32 - n)))) {
      printf("rotr32 %u differs\n", n);
      return 1;
    }
  }
  printf("done\n");
  return 0;
}
