// Stand-alone host program over csrc/keyset_index.h with the plain-memory policy: builds indexes sequentially and compares every
// lookup with a std::map.  Built with -fsanitize=address,undefined by tests/test_keyset_index_sanitize_cpu.py; no device code.
// usage: keyset_index_main [hash seed ...]   (every set below is built and checked under each seed)
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "keyset_index.h"

using key64 = std::array<uint8_t, 64>;
using key32 = std::array<uint8_t, 32>;

static uint64_t g_rng = 0x243f6a8885a308d3ull;
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
  k[32] &= 0x7f;
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

static void words_of(const uint8_t* p, uint32_t* out, int words) { ksi_plain_mem::load_key(p, out, words); }

struct built {
  std::vector<uint8_t> keys;
  std::vector<uint64_t> slots;
  ksi_table t;
  uint32_t occupied = 0, longest = 0;
  bool wrapped = false;
};

// builds the index of `keys` in 2^log2 slots (0: the geometry's choice) and checks it against the maps; `probes`: further
// keys to look up (neighbours, misses)
static void run_set(const char* name, const std::vector<key64>& keys, uint32_t log2, uint64_t seed, const std::vector<key64>& probes,
                    bool want_wrap) {
  uint64_t geo[2];
  const bool ok = ksi_geometry(keys.size(), log2, geo);
  CHECK(ok, "%s: geometry refused", name);
  if (!ok) return;
  built b;
  b.keys.resize(keys.size() * 64);
  for (size_t i = 0; i < keys.size(); ++i) memcpy(&b.keys[i * 64], keys[i].data(), 64);
  b.slots.assign((size_t)geo[0], KSI_EMPTY);
  CHECK(geo[1] == geo[0] * 8 && geo[0] > keys.size() && (geo[0] & (geo[0] - 1)) == 0, "%s: geometry", name);
  b.t = ksi_table{b.slots.data(), (uint32_t)(geo[0] - 1), seed, b.keys.data()};
  std::map<key64, uint32_t> by64;
  std::map<key32, uint32_t> by32;
  for (uint32_t i = 0; i < keys.size(); ++i) {
    bool fresh = false;
    const uint32_t d = ksi_insert<ksi_plain_mem>(b.t, i, &fresh);
    CHECK(d != KSI_NONE && d <= b.t.mask, "%s: insert %u found no slot", name, i);
    const bool first = by64.emplace(keys[i], i).second;
    CHECK(fresh == first, "%s: insert %u fresh=%d, first occurrence=%d", name, i, (int)fresh, (int)first);
    key32 x;
    memcpy(x.data(), keys[i].data(), 32);
    by32.emplace(x, i);
    if (fresh) ++b.occupied;
    if (d != KSI_NONE && d > b.longest) b.longest = d;
  }
  // the table itself: occupied slots = distinct strings, each holding the lowest index of its string; did a chain wrap?
  uint32_t taken = 0;
  for (uint32_t s = 0; s <= b.t.mask; ++s) {
    const uint64_t e = b.slots[s];
    if (e == KSI_EMPTY) continue;
    ++taken;
    const uint32_t idx = (uint32_t)e;
    CHECK(idx < keys.size(), "%s: slot %u holds index %u", name, s, idx);
    if (idx >= keys.size()) continue;
    CHECK(by64.at(keys[idx]) == idx, "%s: slot %u holds index %u, not the lowest of its key", name, s, idx);
    uint32_t w[8], home, tag;
    words_of(keys[idx].data(), w, 8);
    ksi_hash(w, seed, &home, &tag);
    CHECK(tag == (uint32_t)(e >> 32), "%s: slot %u tag", name, s);
    if ((home & b.t.mask) > s) b.wrapped = true;
  }
  CHECK(taken == by64.size() && b.occupied == by64.size(), "%s: %u slots taken, %u fresh inserts, %zu distinct keys", name, taken, b.occupied,
        by64.size());
  CHECK(taken <= b.t.mask, "%s: no empty slot left", name);
  if (want_wrap) CHECK(b.wrapped, "%s: no chain wraps past the last slot under seed %llu", name, (unsigned long long)seed);
  // lookups: every key of the set, the probes, and one-bit neighbours of every key
  auto look = [&](const key64& k) {
    uint32_t w[16];
    words_of(k.data(), w, 16);
    const uint32_t got64 = ksi_lookup64<ksi_plain_mem>(b.t, w), got32 = ksi_lookup32<ksi_plain_mem>(b.t, w);
    const auto it64 = by64.find(k);
    key32 x;
    memcpy(x.data(), k.data(), 32);
    const auto it32 = by32.find(x);
    const uint32_t exp64 = it64 == by64.end() ? KSI_NONE : it64->second, exp32 = it32 == by32.end() ? KSI_NONE : it32->second;
    CHECK(got64 == exp64, "%s: 64-byte lookup gives %u, expected %u", name, got64, exp64);
    CHECK(got32 == exp32, "%s: 32-byte lookup gives %u, expected %u", name, got32, exp32);
  };
  for (const key64& k : keys) {
    look(k);
    key64 n1 = k, n2 = k;
    n1[63] ^= (uint8_t)(1u << (rnd() & 7));      // one bit of the last byte of Y: a 64-byte miss, a 32-byte hit
    n2[0] ^= (uint8_t)(1u << (rnd() & 7));       // one bit of the first byte of X: a miss both ways
    look(n1);
    look(n2);
    look(negated(k));
  }
  for (const key64& k : probes) look(k);
  for (int i = 0; i < 200; ++i) look(random_key());
}

int main(int argc, char** argv) {
  std::vector<uint64_t> seeds;
  for (int i = 1; i < argc; ++i) seeds.push_back(strtoull(argv[i], nullptr, 0));
  if (seeds.empty()) seeds.push_back(0x5ec9u);
  uint64_t geo[2];
  if (!(ksi_geometry(1, 0, geo) && geo[0] == 16 && geo[1] == 128 && ksi_geometry(1000, 0, geo) && geo[0] == 2048 &&
        ksi_geometry(1000, 10, geo) && geo[0] == 1024 && !ksi_geometry(1024, 10, geo) && !ksi_geometry(0, 0, geo) &&
        !ksi_geometry(5, 32, geo))) {
    fprintf(stderr, "FAIL: geometry\n");
    return 1;
  }
  for (const uint64_t seed : seeds) {
    g_rng = 0x243f6a8885a308d3ull;                 // the same keys under every seed
    std::vector<key64> a;
    for (int i = 0; i < 1000; ++i) a.push_back(random_key());
    run_set("1000 keys in 1024 slots", a, 10, seed, {}, /*want_wrap=*/true);
    run_set("1 key in 2 slots", {a[0]}, 1, seed, {a[1], a[2]}, false);
    std::vector<key64> c;
    for (int i = 0; i < 260; ++i) c.push_back(random_key());
    for (int i = 0; i < 40; ++i) {                 // 40 duplicates, spread through the list (duplicates of duplicates included)
      const size_t at = (size_t)(rnd() % c.size());
      c.insert(c.begin() + (long)at, c[(size_t)(rnd() % c.size())]);
    }
    run_set("300 keys, 40 duplicates", c, 0, seed, {}, false);
    run_set("300 keys, 40 duplicates, 512 slots", c, 9, seed, {}, false);
    std::vector<key64> d;
    for (int i = 0; i < 10; ++i) {                 // (X, Y) and (X, p - Y): one home slot, one chain, one tag
      const key64 k = random_key();
      d.push_back(i & 1 ? negated(k) : k);
      d.push_back(random_key());
      d.push_back(i & 1 ? k : negated(k));
    }
    run_set("10 pairs Q / -Q", d, 0, seed, {}, false);
    run_set("10 pairs Q / -Q, 32 slots", d, 5, seed, {}, false);
  }
  if (g_fail) {
    fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  printf("ok %zu seeds\n", seeds.size());
  return 0;
}
