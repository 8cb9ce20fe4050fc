// keyset_index_append_main.cpp - the property s2k_keyset_append rests on, on the host (csrc/keyset_index.h with the
// plain-memory policy; built with AddressSanitizer + UndefinedBehaviorSanitizer by test_keyset_index_append_sanitize_cpu.py):
// an index built over the first part of a key list and then given the rest in ranges of 1, 63 and 65 keys answers, after every
// range, what a brute-force scan of the live keys answers - ksi_lookup64, ksi_lookup32, ksi_lookup33 and ksi_lookup32v, for
// every key of the whole list (live or not yet), their negations, one-bit neighbours and random strings.  The list has
// duplicates across the boundary, Q / -Q pairs across it (same X, the last byte's parity flipped), entries marked "off the
// curve" (validity 0) that share an X with a valid entry on either side of the boundary, and fills the table to one slot short
// of full.  Keys are random bytes: the index never looks at the curve, validity is an array it is handed.
//   usage: keyset_index_append_main SEED [SEED ...]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "keyset_index.h"

namespace {
uint64_t rng_state;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

struct keylist {
  std::vector<uint8_t> keys;    // 64 bytes each
  std::vector<uint8_t> valid;
  size_t size() const { return valid.size(); }
  const uint8_t* at(size_t i) const { return &keys[64 * i]; }
  void push(const uint8_t* k, uint8_t v) {
    keys.insert(keys.end(), k, k + 64);
    valid.push_back(v);
  }
};

uint32_t brute(const keylist& L, size_t live, const uint8_t* q, int nbytes, int parity, bool need_valid) {
  for (size_t i = 0; i < live; ++i) {
    if (memcmp(L.at(i), q, (size_t)nbytes) != 0) continue;
    if (parity >= 0 && (L.at(i)[63] & 1) != parity) continue;
    if (need_valid && !L.valid[i]) continue;
    return (uint32_t)i;
  }
  return KSI_NONE;
}

int fails = 0;
void expect(uint32_t got, uint32_t want, const char* what, size_t live, size_t q) {
  if (got == want) return;
  if (++fails <= 10) fprintf(stderr, "%s: %zu live keys, query %zu: got %u, want %u\n", what, live, q, got, want);
}

void check_all(const ksi_table& t, const keylist& L, size_t live, const std::vector<uint8_t>& queries) {
  const size_t nq = queries.size() / 64;
  for (size_t j = 0; j < nq; ++j) {
    const uint8_t* q = &queries[64 * j];
    uint32_t k[16];
    ksi_plain_mem::load_key(q, k, 16);
    expect(ksi_lookup64<ksi_plain_mem>(t, k), brute(L, live, q, 64, -1, false), "lookup64", live, j);
    expect(ksi_lookup32<ksi_plain_mem>(t, k), brute(L, live, q, 32, -1, false), "lookup32", live, j);
    expect(ksi_lookup32v<ksi_plain_mem>(t, L.valid.data(), k), brute(L, live, q, 32, -1, true), "lookup32v", live, j);
    for (uint32_t prefix = 2; prefix <= 3; ++prefix)
      expect(ksi_lookup33<ksi_plain_mem>(t, L.valid.data(), prefix, k), brute(L, live, q, 32, (int)(prefix & 1), true), "lookup33", live, j);
    expect(ksi_lookup33<ksi_plain_mem>(t, L.valid.data(), 4, k), KSI_NONE, "lookup33 prefix 04", live, j);
  }
}

// slots occupied = distinct 64-byte strings among the live keys
size_t distinct(const keylist& L, size_t live) {
  size_t d = 0;
  for (size_t i = 0; i < live; ++i) d += brute(L, i, L.at(i), 64, -1, false) == KSI_NONE;
  return d;
}

int run(uint64_t seed, uint32_t log2_slots, size_t n_first, const std::vector<size_t>& ranges) {
  rng_state = seed ^ 0x9e3779b97f4a7c15ull;
  size_t total = n_first;
  for (size_t r : ranges) total += r;
  keylist L;
  // the first part: random keys, every 7th marked invalid
  for (size_t i = 0; i < n_first; ++i) {
    uint8_t k[64];
    for (int b = 0; b < 64; ++b) k[b] = (uint8_t)rnd();
    L.push(k, i % 7 != 3);
  }
  // the rest, by kind: fresh key / duplicate of an old key / -Q of an old key / duplicate of an appended key / an invalid
  // entry with the X of an old valid key (another Y, the same parity) / a VALID entry with the X of an old invalid key
  while (L.size() < total) {
    const size_t i = L.size();
    uint8_t k[64];
    const uint32_t kind = rnd() % 8;
    const size_t old = rnd() % n_first, any = rnd() % i;
    uint8_t v = 1;
    if (kind == 1) {
      memcpy(k, L.at(old), 64);
      v = L.valid[old];
    } else if (kind == 2) {
      memcpy(k, L.at(old), 64);
      k[63] ^= 1;                                    // same X, the other parity: a second entry of the chain
      k[40] ^= 0x55;
    } else if (kind == 3) {
      memcpy(k, L.at(any), 64);
      v = L.valid[any];
    } else if (kind == 4) {
      memcpy(k, L.at(old), 64);
      k[50] ^= 2;                                    // same X and parity, not the point: marked invalid
      v = 0;
    } else if (kind == 5 && n_first > 3) {
      const size_t inv = 3 + 7 * (rnd() % ((n_first - 4) / 7 + 1));      // (the first part's invalid entries: 3, 10, ...)
      memcpy(k, L.at(inv), 64);
      k[45] ^= 4;                                    // the real point of an X the first part lists only as an invalid entry
    } else {
      for (int b = 0; b < 64; ++b) k[b] = (uint8_t)rnd();
      v = i % 5 != 0;
    }
    L.push(k, v);
  }
  const size_t nslots = (size_t)1 << log2_slots;
  if (nslots <= total) {
    fprintf(stderr, "2^%u slots for %zu keys\n", log2_slots, total);
    return 1;
  }
  // queries: every key of the whole list, its negation, a one-bit neighbour in Y and in X, and random strings
  std::vector<uint8_t> queries;
  for (size_t i = 0; i < total; ++i) {
    uint8_t q[64];
    memcpy(q, L.at(i), 64);
    queries.insert(queries.end(), q, q + 64);
    q[63] ^= 1;
    queries.insert(queries.end(), q, q + 64);
    q[63] ^= 1;
    q[33 + rnd() % 30] ^= (uint8_t)(1u << (rnd() % 8));
    queries.insert(queries.end(), q, q + 64);
    memcpy(q, L.at(i), 64);
    q[rnd() % 32] ^= (uint8_t)(1u << (rnd() % 8));
    queries.insert(queries.end(), q, q + 64);
    for (int b = 0; b < 64; ++b) q[b] = (uint8_t)rnd();
    queries.insert(queries.end(), q, q + 64);
  }
  std::vector<uint64_t> slots(nslots, KSI_EMPTY);
  const ksi_table t = {slots.data(), (uint32_t)(nslots - 1), seed, L.keys.data()};
  size_t live = 0, occupied = 0;
  std::vector<size_t> steps;
  steps.push_back(n_first);
  steps.insert(steps.end(), ranges.begin(), ranges.end());
  for (size_t step : steps) {
    for (size_t i = live; i < live + step; ++i) {
      bool fresh = false;
      const uint32_t d = ksi_insert<ksi_plain_mem>(t, (uint32_t)i, &fresh);
      if (d == KSI_NONE) {
        fprintf(stderr, "insert of key %zu found no slot\n", i);
        return 1;
      }
      occupied += fresh;
    }
    live += step;
    check_all(t, L, live, queries);
    if (occupied != distinct(L, live)) {
      fprintf(stderr, "%zu live keys: %zu occupied slots, %zu distinct keys\n", live, occupied, distinct(L, live));
      ++fails;
    }
    // no slot names a row that is not live yet
    for (uint64_t e : slots)
      if (e != KSI_EMPTY && (uint32_t)e >= live) {
        fprintf(stderr, "%zu live keys: a slot names key %u\n", live, (uint32_t)e);
        ++fails;
      }
  }
  return fails != 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s SEED [SEED ...]\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; ++a) {
    const uint64_t seed = strtoull(argv[a], nullptr, 0);
    // 37 keys, then ranges of 1, 27, 64, 71 (the device test's steps) in a roomy table; 126 keys, then 1, 63, 65 in a table of
    // 256 slots: one slot stays empty, chains wrap past the last slot; and the same ranges in another order
    if (run(seed, 9, 37, {1, 27, 64, 71})) return 1;
    if (run(seed, 8, 126, {1, 63, 65})) return 1;
    if (run(seed, 8, 126, {65, 1, 63})) return 1;
    if (run(seed, 10, 1, {63, 65, 1})) return 1;
  }
  printf("ok %d seeds\n", argc - 1);
  return 0;
}
