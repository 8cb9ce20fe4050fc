// Stand-alone host program over csrc/keyset_index.h with the plain-memory policy: ksi_lookup33 (33-byte SEC1 compressed keys,
// resolved without a square root) against a brute-force scan of the key list.  Built with -fsanitize=address,undefined by
// tests/test_keyset_index33_sanitize_cpu.py; no device code.
// usage: keyset_index33_main [hash seed ...]   (every set below is built and checked under each seed)
//
// The keys here are random strings: which of them are "valid" is what the validity array says, as it is for the probe.  The
// lists respect the one fact the probe relies on - two VALID keys with the same X and the same parity of Y are the same
// string - and nothing else: invalid keys share X and parity with valid ones, at lower and at higher indices.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "keyset_index.h"

using key64 = std::array<uint8_t, 64>;

static uint64_t g_rng = 0x13198a2e03707344ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static key64 random_key() {
  key64 k;
  for (int i = 0; i < 64; i += 8) {
    const uint64_t v = rnd();
    memcpy(&k[i], &v, 8);
  }
  k[0] &= 0x7f;    // X and Y below p, so that p - Y is a 32-byte string
  k[32] &= 0x7f;   // (0 < Y < p and p is odd: p - Y has the other parity)
  return k;
}
static const uint8_t P_BE[32] = {0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff,
                                 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xfe, 0xff, 0xff, 0xfc, 0x2f};
static key64 negated(const key64& k) {   // (X, p - Y)
  key64 r = k;
  int borrow = 0;
  for (int i = 31; i >= 0; --i) {
    const int d = (int)P_BE[i] - (int)k[32 + i] - borrow;
    r[32 + i] = (uint8_t)(d & 0xff);
    borrow = d < 0;
  }
  return r;
}
// the same X, another Y of the SAME parity: what an off-curve key that a set lists beside the real one looks like to the probe
static key64 same_parity(const key64& k) {
  key64 r = k;
  r[63] ^= (uint8_t)(2u << (rnd() % 7));
  return r;
}

static int g_fail = 0;
#define CHECK(c, ...)                            \
  do {                                           \
    if (!(c)) {                                  \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);              \
      fprintf(stderr, "\n");                     \
      ++g_fail;                                  \
    }                                            \
  } while (0)

struct entry {
  key64 k;
  uint8_t valid;
};

// the definition: the lowest index of a valid key with this X and a Y of the prefix's parity; nothing for another prefix
static uint32_t brute(const std::vector<entry>& set, uint32_t prefix, const uint8_t x[32]) {
  if (prefix != 2 && prefix != 3) return KSI_NONE;
  for (uint32_t i = 0; i < set.size(); ++i)
    if (set[i].valid && memcmp(set[i].k.data(), x, 32) == 0 && (uint32_t)(set[i].k[63] & 1) == (prefix & 1)) return i;
  return KSI_NONE;
}

static void run_set(const char* name, const std::vector<entry>& set, uint32_t log2, uint64_t seed, bool want_one_empty) {
  uint64_t geo[2];
  const bool ok = ksi_geometry(set.size(), log2, geo);
  CHECK(ok, "%s: geometry refused", name);
  if (!ok) return;
  std::vector<uint8_t> keys(set.size() * 64), valid(set.size());
  for (size_t i = 0; i < set.size(); ++i) {
    memcpy(&keys[i * 64], set[i].k.data(), 64);
    valid[i] = set[i].valid;
  }
  std::vector<uint64_t> slots((size_t)geo[0], KSI_EMPTY);
  const ksi_table t = ksi_table{slots.data(), (uint32_t)(geo[0] - 1), seed, keys.data()};
  for (uint32_t i = 0; i < set.size(); ++i) {
    bool fresh = false;
    CHECK(ksi_insert<ksi_plain_mem>(t, i, &fresh) != KSI_NONE, "%s: insert %u found no slot", name, i);
  }
  size_t empty = 0;
  for (const uint64_t e : slots) empty += e == KSI_EMPTY;
  CHECK(empty >= 1, "%s: no empty slot", name);
  if (want_one_empty) CHECK(empty == 1, "%s: %zu empty slots, wanted exactly one", name, empty);
  size_t hits = 0, looks = 0;
  auto look = [&](uint32_t prefix, const uint8_t* x) {
    uint32_t w[8];
    ksi_plain_mem::load_key(x, w, 8);
    const uint32_t got = ksi_lookup33<ksi_plain_mem>(t, valid.data(), prefix, w), exp = brute(set, prefix, x);
    CHECK(got == exp, "%s: prefix %02x gives %u, expected %u", name, prefix, got, exp);
    hits += got != KSI_NONE;
    ++looks;
  };
  static const uint32_t prefixes[] = {0x02, 0x03, 0x00, 0x04, 0x05};
  for (const entry& e : set) {
    for (const uint32_t p : prefixes) look(p, e.k.data());
    key64 n = e.k;                                    // X one bit away from a stored X
    const unsigned bit = (unsigned)(rnd() % 256);
    n[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    look(2, n.data());
    look(3, n.data());
  }
  for (int i = 0; i < 100; ++i) {
    const key64 r = random_key();
    look(2 + (uint32_t)(i & 1), r.data());
  }
  CHECK(hits > 0 && hits < looks, "%s: %zu hits in %zu lookups", name, hits, looks);
}

int main(int argc, char** argv) {
  std::vector<uint64_t> seeds;
  for (int i = 1; i < argc; ++i) seeds.push_back(strtoull(argv[i], nullptr, 0));
  if (seeds.empty()) seeds.push_back(0x5ec9u);
  for (const uint64_t seed : seeds) {
    g_rng = 0x13198a2e03707344ull;                 // the same keys under every seed
    std::vector<entry> a;
    for (int i = 0; i < 60; ++i) {
      const key64 q = random_key();
      switch (i % 6) {
        case 0:                                    // Q and -Q, both valid, in either order
          a.push_back({i & 1 ? negated(q) : q, 1});
          a.push_back({random_key(), 1});
          a.push_back({i & 1 ? q : negated(q), 1});
          break;
        case 1:                                    // an invalid key with Q's X and parity BEFORE Q
          a.push_back({same_parity(q), 0});
          a.push_back({q, 1});
          break;
        case 2:                                    // ... and AFTER Q, with -Q between them
          a.push_back({q, 1});
          a.push_back({negated(q), 1});
          a.push_back({same_parity(q), 0});
          break;
        case 3:                                    // an invalid key alone on its X
          a.push_back({q, 0});
          break;
        case 4:                                    // invalid keys of both parities around a valid one, and nothing valid of the other parity
          a.push_back({same_parity(negated(q)), 0});
          a.push_back({same_parity(q), 0});
          a.push_back({q, 1});
          a.push_back({same_parity(q), 0});
          break;
        default:
          a.push_back({q, 1});
      }
    }
    for (int i = 0; i < 25; ++i) {                 // duplicates of valid and of invalid keys, spread through the list
      const entry e = a[(size_t)(rnd() % a.size())];
      a.insert(a.begin() + (long)(rnd() % a.size()), e);
    }
    run_set("traps, pairs and duplicates", a, 0, seed, false);
    run_set("traps, pairs and duplicates, nearly full", a, 8, seed, false);
    // a table with ONE empty slot: 2^k - 1 distinct strings in 2^k slots (the duplicates above would leave more)
    std::vector<entry> c;
    for (const entry& e : a) {
      bool seen = false;
      for (const entry& f : c) seen = seen || f.k == e.k;
      if (!seen && c.size() < 63) c.push_back(e);
    }
    while (c.size() < 63) c.push_back({random_key(), (uint8_t)(c.size() & 1)});
    run_set("63 distinct keys in 64 slots", c, 6, seed, true);
    run_set("1 key in 2 slots", {a[0]}, 1, seed, true);
  }
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok %zu seeds\n", seeds.size());
  return 0;
}
