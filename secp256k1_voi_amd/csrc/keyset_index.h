// keyset_index.h — the index of a key set: key bytes -> key index (s2k_keyset_index_create, s2k_keyset_lookup*).
// Shared by the device (keyset_index.hip: k_ksi_build, k_ksi_lookup; ingest.hip: k_parse_encoded_keyset) and by host programs
// (tests/c/keyset_index_main.cpp, tests/c/keyset_index33_main.cpp, tests/c/keyset_index32v_main.cpp):
// the probe and insert steps are written once over a small memory-access policy M, which on the device is atomics and
// vector loads and on the host plain loads and stores.
//
// An open-addressing table with linear probing and no deletions.
//   slot    one uint64_t: tag in the high word, key index in the low word; EMPTY = all ones (a key index is at most
//           KSI_MAX_KEYS = 0x0fffffff, so an occupied slot is never all ones).
//   hash    the chained mix32 over the eight words of X ONLY, seeded per set (the construction of k_key_insert<32>, keyed.hip,
//           and for its reason: the difference two strings leave in the state depends on the state before it, so no pair of
//           byte strings collides for every seed).  The home slot and the tag are two different final mixes of that state.
//           Hashing X alone lets one table serve 64-byte (X || Y) and 32-byte (x-only) lookups: Q and -Q share a home slot,
//           a chain and a tag, and are told apart by the comparison of all 64 bytes.
//   INVARIANT   a slot, once taken, belongs to ONE 64-byte string forever; only its index can go down (ksi_insert step 2).
//           So concurrent inserts and later lookups never see a chain change shape, and duplicates of a key merge into one
//           slot that ends up holding their lowest index, whatever the order of the inserts.
//   bounds  the host keeps slots = 2^log2_slots > n_keys, so at least one slot stays empty; on top of that EVERY probe loop
//           below runs at most `slots` iterations: a lookup that exhausts them reports a miss, an insert KSI_NONE.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KSI_FN __host__ __device__ inline
#else
#define KSI_FN inline
#endif

constexpr uint64_t KSI_EMPTY = ~(uint64_t)0;
constexpr uint32_t KSI_NONE = 0xffffffffu;        // lookup: no key of the set; insert: the probe bound ran out
constexpr uint32_t KSI_MAX_KEYS = 0x0fffffffu;    // (s2k_keyset_create_ex's cap)
constexpr uint32_t KSI_MAX_LOG2 = 31;

KSI_FN uint32_t ksi_mix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h;
}

// x: the 32 bytes of X as eight little-endian words, in memory order
KSI_FN void ksi_hash(const uint32_t x[8], uint64_t seed, uint32_t* home, uint32_t* tag) {
  uint32_t h = (uint32_t)seed;
  for (int i = 0; i < 8; ++i) h = ksi_mix32(h ^ x[i]);
  h ^= (uint32_t)(seed >> 32);
  *home = ksi_mix32(h);
  *tag = ksi_mix32(h ^ 0x9e3779b9u);
}

KSI_FN bool ksi_same(const uint32_t* a, const uint32_t* b, int words) {
  uint32_t diff = 0;
  for (int i = 0; i < words; ++i) diff |= a[i] ^ b[i];
  return diff == 0;
}

// the table as the probe loops see it: slots[mask + 1], the seed, and the key array of the set (64 bytes per key)
struct ksi_table {
  uint64_t* slots;
  uint32_t mask;
  uint64_t seed;
  const uint8_t* keys;
};

// Policy M:
//   static uint64_t load(const uint64_t* p)                          a slot as it is now
//   static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v)    compare-and-swap, returns what was there
//   static void     min_u64(uint64_t* p, uint64_t v)                 *p = min(*p, v)
//   static void     load_key(const uint8_t* p, uint32_t* out, int words)   the first `words` words of a key OF THE SET

// Insert of key i of the set.  Returns the probe distance of the slot the key lives in (0: its home slot), KSI_NONE when
// the bound ran out (cannot happen while slots > n_keys); *fresh: this call took an empty slot (a distinct 64-byte string).
template <class M>
KSI_FN uint32_t ksi_insert(const ksi_table& t, uint32_t i, bool* fresh) {
  uint32_t k[16], home, tag;
  M::load_key(t.keys + (size_t)i * 64, k, 16);
  ksi_hash(k, t.seed, &home, &tag);
  const uint64_t mine = ((uint64_t)tag << 32) | i;
  uint32_t s = home & t.mask;
  *fresh = false;
  for (uint32_t d = 0; d <= t.mask; ++d) {
    uint64_t old = M::load(&t.slots[s]);
    // 1. empty: take it.  A lost race leaves the winner's entry in `old`: the SAME slot is looked at again, below
    if (old == KSI_EMPTY) {
      old = M::cas(&t.slots[s], KSI_EMPTY, mine);
      if (old == KSI_EMPTY) {
        *fresh = true;
        return d;
      }
    }
    // 2. taken by this very string (the stored index may be going down meanwhile: every index the slot ever holds names
    //    the same 64 bytes): the lowest index stays
    if ((uint32_t)(old >> 32) == tag) {
      uint32_t o[16];
      M::load_key(t.keys + (size_t)(uint32_t)old * 64, o, 16);
      if (ksi_same(k, o, 16)) {
        M::min_u64(&t.slots[s], mine);
        return d;
      }
    }
    // 3. another string's slot
    s = (s + 1) & t.mask;
  }
  return KSI_NONE;
}

// k: the looked-up key as sixteen little-endian words (X || Y).  The index of the set's key with these 64 bytes (the lowest
// one when the set lists it several times), or KSI_NONE.
template <class M>
KSI_FN uint32_t ksi_lookup64(const ksi_table& t, const uint32_t k[16]) {
  uint32_t home, tag;
  ksi_hash(k, t.seed, &home, &tag);
  uint32_t s = home & t.mask;
  for (uint32_t d = 0; d <= t.mask; ++d) {
    const uint64_t e = M::load(&t.slots[s]);
    if (e == KSI_EMPTY) return KSI_NONE;
    if ((uint32_t)(e >> 32) == tag) {
      uint32_t o[16];
      M::load_key(t.keys + (size_t)(uint32_t)e * 64, o, 16);
      if (ksi_same(k, o, 16)) return (uint32_t)e;
    }
    s = (s + 1) & t.mask;
  }
  return KSI_NONE;
}

// x: eight words.  The LOWEST index of a key of the set whose X is x (Q and -Q are two entries of one chain, and the x-only
// key stands for both), or KSI_NONE: the walk goes on to the empty slot.
template <class M>
KSI_FN uint32_t ksi_lookup32(const ksi_table& t, const uint32_t x[8]) {
  uint32_t home, tag, best = KSI_NONE;
  ksi_hash(x, t.seed, &home, &tag);
  uint32_t s = home & t.mask;
  for (uint32_t d = 0; d <= t.mask; ++d) {
    const uint64_t e = M::load(&t.slots[s]);
    if (e == KSI_EMPTY) break;
    if ((uint32_t)(e >> 32) == tag && (uint32_t)e < best) {
      uint32_t o[8];
      M::load_key(t.keys + (size_t)(uint32_t)e * 64, o, 8);
      if (ksi_same(x, o, 8)) best = (uint32_t)e;
    }
    s = (s + 1) & t.mask;
  }
  return best;
}

// A 33-byte SEC1 compressed key `prefix || X` (x: the eight words of X): the index ksi_lookup64 would give for the point the
// bytes decode to (SetCompressedBytes), or KSI_NONE - the bytes decode to nothing, or the set does not hold that point.  No
// square root is taken: the walk over the chain of X keeps the LOWEST index of an entry with this X, a Y of the asked parity
// (byte 63 of the key, bit 0) and a non-zero byte in `valid` (the set's validity array, one byte per key: canonical
// coordinates on the curve).  A valid key with a given X and parity is unique, so such an entry IS the decoded point; a set
// may also list (X, Y') off the curve with the same parity, which is not that point and is never answered.  A prefix other
// than 02 / 03 matches nothing, and neither does an X >= p or an X with X^3 + 7 not a square: no valid key has such an X.
template <class M>
KSI_FN uint32_t ksi_lookup33(const ksi_table& t, const uint8_t* valid, uint32_t prefix, const uint32_t x[8]) {
  if (prefix != 2u && prefix != 3u) return KSI_NONE;
  uint32_t home, tag, best = KSI_NONE;
  ksi_hash(x, t.seed, &home, &tag);
  uint32_t s = home & t.mask;
  for (uint32_t d = 0; d <= t.mask; ++d) {
    const uint64_t e = M::load(&t.slots[s]);
    if (e == KSI_EMPTY) break;
    if ((uint32_t)(e >> 32) == tag && (uint32_t)e < best) {
      uint32_t o[16];
      M::load_key(t.keys + (size_t)(uint32_t)e * 64, o, 16);
      if (ksi_same(x, o, 8) && ((o[15] >> 24) & 1u) == (prefix & 1u) && valid[(uint32_t)e] != 0) best = (uint32_t)e;
    }
    s = (s + 1) & t.mask;
  }
  return best;
}

// An x-only key (BIP-340; x: the eight words of X) among the VALID keys of the set: the LOWEST index of an entry with this X and
// a non-zero byte in `valid`, or KSI_NONE.  ksi_lookup32 answers an entry that is no point as readily as one that is; a
// caller that goes on to verify under lift_x(X) on the set's tables (s2k_schnorr_verify_batch_keyset_bykey) must not be
// handed (X, Y') off the curve where X itself lifts - that entry is skipped here, whether the real (X, Y) follows it, comes
// before it or is missing.  Either parity of Y serves: X stands for Q and -Q alike and the set's ladders flip the half
// scalars' signs under an odd Y.  An X >= p or an X with X^3 + 7 not a square matches nothing (no valid key has such an X);
// no square root is taken.
template <class M>
KSI_FN uint32_t ksi_lookup32v(const ksi_table& t, const uint8_t* valid, const uint32_t x[8]) {
  uint32_t home, tag, best = KSI_NONE;
  ksi_hash(x, t.seed, &home, &tag);
  uint32_t s = home & t.mask;
  for (uint32_t d = 0; d <= t.mask; ++d) {
    const uint64_t e = M::load(&t.slots[s]);
    if (e == KSI_EMPTY) break;
    if ((uint32_t)(e >> 32) == tag && (uint32_t)e < best) {
      uint32_t o[8];
      M::load_key(t.keys + (size_t)(uint32_t)e * 64, o, 8);
      if (ksi_same(x, o, 8) && valid[(uint32_t)e] != 0) best = (uint32_t)e;
    }
    s = (s + 1) & t.mask;
  }
  return best;
}

// s2k_keyset_index_geometry: out ={slots, bytes}; log2_slots 0 = the power of two >= 2 n_keys, at least 16.  False: refused.
inline bool ksi_geometry(size_t n_keys, uint32_t log2_slots, uint64_t out[2]) {
  if (n_keys == 0 || n_keys > KSI_MAX_KEYS || log2_slots > KSI_MAX_LOG2) return false;
  if (log2_slots == 0) {
    log2_slots = 4;
    while (((uint64_t)1 << log2_slots) < 2 * (uint64_t)n_keys) ++log2_slots;
  }
  const uint64_t slots = (uint64_t)1 << log2_slots;
  if (slots <= n_keys) return false;
  out[0] = slots;
  out[1] = slots * sizeof(uint64_t);
  return true;
}

// plain memory: one thread (host programs, and the reference a test compares the device against)
struct ksi_plain_mem {
  static uint64_t load(const uint64_t* p) { return *p; }
  static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
    const uint64_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static void min_u64(uint64_t* p, uint64_t v) {
    if (v < *p) *p = v;
  }
  static void load_key(const uint8_t* p, uint32_t* out, int words) {
    for (int i = 0; i < words; ++i)
      out[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
  }
};

#if defined(__HIPCC__)
// device memory: many lanes at once (keyset_index.hip: build and lookup kernels; ingest.hip: the key-set parse kernel)
struct ksi_dev_mem {
  static __device__ __forceinline__ uint64_t load(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
    return atomicCAS(reinterpret_cast<unsigned long long*>(p), (unsigned long long)expect, (unsigned long long)v);
  }
  static __device__ __forceinline__ void min_u64(uint64_t* p, uint64_t v) {
    (void)atomicMin(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
  }
  // a key of the set: 64 bytes at a multiple of 64 from a 256-byte aligned base
  static __device__ __forceinline__ void load_key(const uint8_t* p, uint32_t* out, int words) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * i >= words) break;
      const uint4 v = q[i];
      out[4 * i] = v.x;
      out[4 * i + 1] = v.y;
      out[4 * i + 2] = v.z;
      out[4 * i + 3] = v.w;
    }
  }
};
#endif
