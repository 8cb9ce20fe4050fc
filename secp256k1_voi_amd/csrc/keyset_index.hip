// keyset_index.hip — the index of a key set on the device: key bytes -> key index (keyset_index.h has the table and its
// probe loops; engine.hip owns the set and the calls: s2k_keyset_index_create, s2k_keyset_lookup*,
// s2k_ecdsa_verify_batch_keyset_bykey*).
//   k_ksi_build    one lane per key of a range of the set (all of it at creation, the new keys at s2k_keyset_append):
//                  ksi_insert with atomics; counts the occupied slots (= distinct 64-byte keys) and keeps the longest probe
//                  distance of a stored entry, both going on from what earlier ranges left in `info`
//   k_ksi_lookup   one lane per looked-up key, read with the caller's stride: 64 bytes (X || Y), 32 (X) or 33 (SEC1
//                  compressed: prefix || X, resolved without a square root - ksi_lookup33), or 32 bytes of X among the set's
//                  valid keys only (S2K_KSI_X_VALID: ksi_lookup32v, the lookup of s2k_schnorr_verify_batch_keyset_bykey)
#include "engine_internal.h"
#include "keyset_index.h"

namespace {

__global__ void __launch_bounds__(256)
k_ksi_build(uint32_t first, uint32_t count, ksi_table t, uint32_t* __restrict__ info) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool fresh = false;
  uint32_t d = 0;
  if (i < count) {
    d = ksi_insert<ksi_dev_mem>(t, first + i, &fresh);
    if (d == KSI_NONE) {
      atomicOr(&info[S2K_KSI_FAILED], 1u);
      d = 0;
    }
  }
  // the two counters, once per wave (every lane of the wave is here: lanes past the last key count nothing)
  const uint32_t nfresh = (uint32_t)__popcll(__ballot(fresh));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t v = __shfl_xor(d, o, 64);
    d = v > d ? v : d;
  }
  if ((threadIdx.x & 63u) == 0) {
    if (nfresh) atomicAdd(&info[S2K_KSI_OCCUPIED], nfresh);
    if (d) atomicMax(&info[S2K_KSI_LONGEST], d);
  }
}

// WORDS little-endian words of a looked-up key at any address: quads when `wide` (base and stride multiples of 16), words
// when `aligned4` (multiples of 4), else bytes (65-byte records read from their second byte)
template <int WORDS>
S2K_DEV void ksi_load_query(const uint8_t* p, bool wide, bool aligned4, uint32_t out[WORDS]) {
  if (wide) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < WORDS / 4; ++i) {
      const uint4 v = q[i];
      out[4 * i] = v.x;
      out[4 * i + 1] = v.y;
      out[4 * i + 2] = v.z;
      out[4 * i + 3] = v.w;
    }
  } else if (aligned4) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < WORDS; ++i) out[i] = q[i];
  } else {
#pragma unroll
    for (int i = 0; i < WORDS; ++i)
      out[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
  }
}

// KEYBYTES S2K_KSI_X_VALID: 32 bytes, answered by ksi_lookup32v
template <int KEYBYTES>
__global__ void __launch_bounds__(256)
k_ksi_lookup(uint32_t n, const uint8_t* __restrict__ q, size_t stride, bool wide, bool aligned4, ksi_table t,
             const uint8_t* __restrict__ key_valid, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr int NBYTES = KEYBYTES == S2K_KSI_X_VALID ? 32 : KEYBYTES;
  uint32_t k[NBYTES / 4];
  if constexpr (KEYBYTES == 33) {
    // the prefix byte, then X from the second byte: bytes, whatever the stride (33 is aligned to nothing)
    const uint8_t* p = q + (size_t)i * stride;
    ksi_load_query<8>(p + 1, false, false, k);
    out[i] = ksi_lookup33<ksi_dev_mem>(t, key_valid, p[0], k);
  } else if constexpr (KEYBYTES == S2K_KSI_X_VALID) {
    ksi_load_query<8>(q + (size_t)i * stride, wide, aligned4, k);
    out[i] = ksi_lookup32v<ksi_dev_mem>(t, key_valid, k);
  } else {
    ksi_load_query<KEYBYTES / 4>(q + (size_t)i * stride, wide, aligned4, k);
    out[i] = KEYBYTES == 64 ? ksi_lookup64<ksi_dev_mem>(t, k) : ksi_lookup32<ksi_dev_mem>(t, k);
  }
}
}  // namespace

// inserts the keys first .. first + count - 1 of the set.  first = 0: slots (2^log2_slots entries) all KSI_EMPTY and info
// (S2K_KSI_INFO_WORDS words) all zero, both set by the caller on `st`; first > 0: the table holds the keys below `first`
__attribute__((visibility("hidden"))) int s2k_internal_ksi_build(s2k_ctx* ctx, hipStream_t st, const uint8_t* set_keys, size_t first, size_t count,
                                                                 uint64_t* slots, uint32_t log2_slots, uint64_t seed, uint32_t* info) {
  const size_t nkeys = first + count;
  if (count == 0 || nkeys > KSI_MAX_KEYS || log2_slots > KSI_MAX_LOG2 || ((uint64_t)1 << log2_slots) <= nkeys)
    return fail(ctx, S2K_ERR_ARG, "key-set index of %zu keys in 2^%u slots", nkeys, log2_slots);
  const ksi_table t = {slots, (uint32_t)(((uint64_t)1 << log2_slots) - 1), seed, set_keys};
  k_ksi_build<<<blocks_for(count), 256, 0, st>>>((uint32_t)first, (uint32_t)count, t, info);
  HIP_TRY(ctx, hipGetLastError());
  return S2K_OK;
}

// d_out[i] = index of the set's key equal to the key_bytes bytes at d_keys + i * stride, or KSI_NONE (enqueue only);
// key_valid: the set's validity bytes (read for key_bytes 33 and S2K_KSI_X_VALID only)
__attribute__((visibility("hidden"))) int s2k_internal_ksi_lookup(s2k_ctx* ctx, hipStream_t st, const uint8_t* set_keys, const uint64_t* slots,
                                                                  uint32_t log2_slots, uint64_t seed, const uint8_t* key_valid, size_t n,
                                                                  const uint8_t* d_keys, int key_bytes, size_t stride, uint32_t* d_out) {
  const int nbytes = key_bytes == S2K_KSI_X_VALID ? 32 : key_bytes;
  if ((nbytes != 64 && nbytes != 32 && nbytes != 33) || stride < (size_t)nbytes || n >= S2K_MAX_BATCH || log2_slots > KSI_MAX_LOG2)
    return fail(ctx, S2K_ERR_ARG, "key-set lookup: %zu keys of %d bytes at stride %zu", n, nbytes, stride);
  if (n == 0) return S2K_OK;
  const ksi_table t = {const_cast<uint64_t*>(slots), (uint32_t)(((uint64_t)1 << log2_slots) - 1), seed, set_keys};
  const uintptr_t both = (uintptr_t)d_keys | (uintptr_t)stride;
  const bool wide = (both & 15u) == 0, aligned4 = (both & 3u) == 0;
  if (key_bytes == 64) k_ksi_lookup<64><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, d_keys, stride, wide, aligned4, t, key_valid, d_out);
  else if (key_bytes == 32) k_ksi_lookup<32><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, d_keys, stride, wide, aligned4, t, key_valid, d_out);
  else if (key_bytes == S2K_KSI_X_VALID)
    k_ksi_lookup<S2K_KSI_X_VALID><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, d_keys, stride, wide, aligned4, t, key_valid, d_out);
  else k_ksi_lookup<33><<<blocks_for(n), 256, 0, st>>>((uint32_t)n, d_keys, stride, false, false, t, key_valid, d_out);
  HIP_TRY(ctx, hipGetLastError());
  return S2K_OK;
}
