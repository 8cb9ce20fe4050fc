// The host half of hashing to the curve (csrc/h2c_host.h: SHA-256 and DST_prime, both of which take caller-supplied
// lengths) under AddressSanitizer + UBSan.  Every input lives in a heap buffer of its exact length, so one byte read past
// the end is a report; outputs go to exact-size heap buffers too.  Checked against known answers: the FIPS 180-4 examples,
// the two DST_prime values of RFC 9380 K.1 / K.2, and chunked against one-shot hashing for every split of 0..300 bytes.
// Built host-only (g++ -fsanitize=address,undefined) and run on the CPU.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "h2c_host.h"

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t i = 0; i < n; ++i) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}

static std::string sha_hex(const uint8_t* p, size_t n, size_t chunk) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);   // exact size: overreads trip ASan
  if (n) memcpy(in, p, n);
  uint8_t* out = (uint8_t*)malloc(32);
  s2k_h2c::sha256 h;
  if (chunk == 0) {
    h.update(in, n);
  } else {
    for (size_t at = 0; at < n; at += chunk) h.update(in + at, n - at < chunk ? n - at : chunk);
  }
  h.final(out);
  std::string s = hex(out, 32);
  free(out);
  free(in);
  return s;
}

static std::string dst_prime_hex(const uint8_t* p, size_t n) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(in, p, n);
  uint8_t* out = (uint8_t*)malloc(256);
  size_t len = s2k_h2c::dst_prime(in, n, out);
  std::string s = hex(out, len);
  free(out);
  free(in);
  return s;
}

#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #c);          \
      return 1;                                              \
    }                                                        \
  } while (0)

int main() {
  size_t runs = 0;
  CHECK(sha_hex((const uint8_t*)"", 0, 0) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
  CHECK(sha_hex((const uint8_t*)"abc", 3, 0) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
  const char* two = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";
  CHECK(sha_hex((const uint8_t*)two, strlen(two), 0) == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");
  std::vector<uint8_t> m(300);
  for (size_t i = 0; i < m.size(); ++i) m[i] = (uint8_t)(i * 131 + 7);
  for (size_t n = 0; n <= m.size(); ++n) {                   // every padding residue, every way to feed it
    const std::string want = sha_hex(m.data(), n, 0);
    for (size_t chunk : {(size_t)1, (size_t)3, (size_t)63, (size_t)64, (size_t)65, (size_t)127}) {
      CHECK(sha_hex(m.data(), n, chunk) == want);
      ++runs;
    }
  }
  // DST_prime: RFC 9380 K.1 (38 bytes) and K.2 (256 bytes: hashed), then every length around the limits
  const std::string k1 = "QUUX-V01-CS02-with-expander-SHA256-128";
  CHECK(dst_prime_hex((const uint8_t*)k1.data(), k1.size()) == "515555582d5630312d435330322d776974682d657870616e6465722d5348413235362d31323826");
  const std::string k2 = k1 + "-long-DST-" + std::string(208, '1');
  CHECK(k2.size() == 256);
  CHECK(dst_prime_hex((const uint8_t*)k2.data(), k2.size()) == "412717974da474d0f8c420f320ff81e8432adb7c927d9bd082b4fb4d16c0a23620");
  CHECK(dst_prime_hex(m.data(), 0) == "");
  {
    uint8_t out[256];
    CHECK(s2k_h2c::dst_prime(nullptr, 5, out) == 0);
  }
  for (size_t n = 1; n <= m.size(); ++n) {
    const std::string got = dst_prime_hex(m.data(), n);
    if (n <= 255) {
      CHECK(got.size() == 2 * (n + 1) && got.substr(0, 2 * n) == hex(m.data(), n) && strtoul(got.substr(2 * n).c_str(), nullptr, 16) == n);
    } else {
      std::vector<uint8_t> t(17 + n);
      memcpy(t.data(), "H2C-OVERSIZE-DST-", 17);
      memcpy(t.data() + 17, m.data(), n);
      CHECK(got == sha_hex(t.data(), t.size(), 0) + "20");
    }
    ++runs;
  }
  printf("ok %zu inputs\n", runs);
  return 0;
}
