// Stand-alone host program over csrc/keyset_index.h with the plain-memory policy: ksi_lookup32v (an x-only key among the VALID
// keys of a set) against a brute-force scan of the key list.  Built with -fsanitize=address,undefined by
// tests/test_keyset_index32v_cpu.py; no device code.
// usage: keyset_index32v_main SET_FILE [hash seed ...]   (the set is indexed and checked under each seed)
//
// SET_FILE (written by the test, which makes real points with its own affine arithmetic and says which entries are valid
// public keys): a little-endian uint32 count n, n keys of 64 bytes (X || Y, big-endian coordinates), n validity bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "keyset_index.h"

static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
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

struct key_set {
  std::vector<uint8_t> keys, valid;
  size_t n() const { return valid.size(); }
};

// the definition: the lowest index of a valid key with this X
static uint32_t brute(const key_set& set, const uint8_t x[32]) {
  for (uint32_t i = 0; i < set.n(); ++i)
    if (set.valid[i] && memcmp(&set.keys[(size_t)i * 64], x, 32) == 0) return i;
  return KSI_NONE;
}
// ... and of any key with this X, valid or not: what ksi_lookup32 answers
static uint32_t brute_any(const key_set& set, const uint8_t x[32]) {
  for (uint32_t i = 0; i < set.n(); ++i)
    if (memcmp(&set.keys[(size_t)i * 64], x, 32) == 0) return i;
  return KSI_NONE;
}

static void run_set(const char* name, const key_set& set, uint32_t log2, uint64_t seed) {
  uint64_t geo[2];
  const bool ok = ksi_geometry(set.n(), log2, geo);
  CHECK(ok, "%s: geometry refused", name);
  if (!ok) return;
  std::vector<uint64_t> slots((size_t)geo[0], KSI_EMPTY);
  const ksi_table t = ksi_table{slots.data(), (uint32_t)(geo[0] - 1), seed, set.keys.data()};
  for (uint32_t i = 0; i < set.n(); ++i) {
    bool fresh = false;
    CHECK(ksi_insert<ksi_plain_mem>(t, i, &fresh) != KSI_NONE, "%s: insert %u found no slot", name, i);
  }
  size_t empty = 0;
  for (const uint64_t e : slots) empty += e == KSI_EMPTY;
  CHECK(empty >= 1, "%s: no empty slot", name);
  size_t hits = 0, looks = 0, differs = 0;
  auto look = [&](const uint8_t* x) {
    uint32_t w[8];
    ksi_plain_mem::load_key(x, w, 8);
    const uint32_t got = ksi_lookup32v<ksi_plain_mem>(t, set.valid.data(), w), exp = brute(set, x);
    CHECK(got == exp, "%s: the valid-only lookup gives %u, expected %u", name, got, exp);
    const uint32_t any = ksi_lookup32<ksi_plain_mem>(t, w), exp_any = brute_any(set, x);
    CHECK(any == exp_any, "%s: the lookup of any entry gives %u, expected %u", name, any, exp_any);
    CHECK(got == KSI_NONE || set.valid[got], "%s: entry %u is answered and is not valid", name, got);
    hits += got != KSI_NONE;
    differs += got != any;
    ++looks;
  };
  for (uint32_t i = 0; i < set.n(); ++i) {
    const uint8_t* k = &set.keys[(size_t)i * 64];
    look(k);
    uint8_t nb[32];                                    // X one bit away from a stored X
    memcpy(nb, k, 32);
    const unsigned bit = (unsigned)(rnd() % 256);
    nb[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    look(nb);
  }
  for (int i = 0; i < 200; ++i) {
    uint8_t r[32];
    for (int j = 0; j < 32; j += 8) {
      const uint64_t v = rnd();
      memcpy(&r[j], &v, 8);
    }
    if (i & 1) memset(r, 0xff, 20);                    // X >= p
    look(r);
  }
  CHECK(hits > 0 && hits < looks, "%s: %zu hits in %zu lookups", name, hits, looks);
  // (the set holds entries that are no keys: there the two lookups part - an index against a miss, or a lower index against the valid one)
  CHECK(differs > 0, "%s: the valid-only lookup never differs from the lookup of any entry", name);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s SET_FILE [hash seed ...]\n", argv[0]);
    return 2;
  }
  key_set set;
  {
    FILE* f = fopen(argv[1], "rb");
    uint8_t hdr[4];
    if (!f || fread(hdr, 1, 4, f) != 4) {
      fprintf(stderr, "cannot read %s\n", argv[1]);
      return 2;
    }
    const size_t n = (size_t)hdr[0] | ((size_t)hdr[1] << 8) | ((size_t)hdr[2] << 16) | ((size_t)hdr[3] << 24);
    if (n == 0 || n > 100000) {
      fprintf(stderr, "%s: %zu keys\n", argv[1], n);
      return 2;
    }
    set.keys.resize(n * 64);
    set.valid.resize(n);
    const bool ok = fread(set.keys.data(), 1, n * 64, f) == n * 64 && fread(set.valid.data(), 1, n, f) == n;
    fclose(f);
    if (!ok) {
      fprintf(stderr, "%s: short file\n", argv[1]);
      return 2;
    }
  }
  std::vector<uint64_t> seeds;
  for (int i = 2; i < argc; ++i) seeds.push_back(strtoull(argv[i], nullptr, 0));
  if (seeds.empty()) seeds.push_back(0x5ec9u);
  uint32_t tight = 1;                                  // slots = the next power of two above the number of keys
  while (((size_t)1 << tight) <= set.n()) ++tight;
  key_set one;
  for (size_t i = 0; i < set.n() && one.n() == 0; ++i)
    if (!set.valid[i]) {                               // a set of one entry, invalid: every lookup misses, one finds the entry
      one.keys.assign(&set.keys[i * 64], &set.keys[i * 64] + 64);
      one.valid.assign(1, 0);
    }
  for (const uint64_t seed : seeds) {
    g_rng = 0x243f6a8885a308d3ull;
    run_set("the set, automatic geometry", set, 0, seed);
    run_set("the set, nearly full", set, tight, seed);
    if (one.n()) {
      uint64_t geo[2];
      std::vector<uint64_t> slots(2, KSI_EMPTY);
      CHECK(ksi_geometry(1, 1, geo) && geo[0] == 2, "one key in two slots: geometry");
      const ksi_table t = ksi_table{slots.data(), 1u, seed, one.keys.data()};
      bool fresh = false;
      CHECK(ksi_insert<ksi_plain_mem>(t, 0, &fresh) != KSI_NONE && fresh, "one key in two slots: insert");
      uint32_t w[8];
      ksi_plain_mem::load_key(one.keys.data(), w, 8);
      CHECK(ksi_lookup32<ksi_plain_mem>(t, w) == 0, "one invalid key: the lookup of any entry finds it");
      CHECK(ksi_lookup32v<ksi_plain_mem>(t, one.valid.data(), w) == KSI_NONE, "one invalid key: the valid-only lookup misses");
    }
  }
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok %zu seeds, %zu keys\n", seeds.size(), set.n());
  return 0;
}
