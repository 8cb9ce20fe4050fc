// digest.hip — SHA-2 and Keccak message digests on the device, batched, and the ECDSA verification calls that take messages.
// The reference's ECDSA callers start from (message, hash): h := sha256.Sum256(m); pk.Verify(h[:], sig, opts)
// (secec/ecdsa.go:171-228; a hash longer than 32 bytes gives its leftmost 32 bytes to the scalar, hashToScalar, :477-486).
// Every other ECDSA entry point here takes the digest; these hash first, on the device: k_digest_messages writes the
// digests into a buffer of the context (s2k_ctx::msg_digest, 32 bytes per item) and the digest sibling's device form runs
// behind it on the same stream, unchanged - so the verdicts are the sibling's on the digests of the messages, on whatever
// ladder its dispatch picks.
//
// One lane per message, 256 lanes per workgroup.  A workgroup's 256 messages are one contiguous stretch of the blob: it is
// copied into LDS with aligned 16-byte loads when it fits DG_CAP, and read in place otherwise (the rule of pe_stage,
// ingest.hip; the twin here aligns the ADDRESS, not the offset, so a caller's device blob may start anywhere - an aligned
// 16-byte load that holds one byte of the stretch never leaves that byte's page).  Lanes of a wave with different block
// counts run to the longest of them: a batch with one very long message is slow, not wrong.  Public data only.
//
// Two kernels over the same staging, item addressing and output rows (dg_locate): k_digest_messages for the SHA-2 ids and
// k_digest_keccak for S2K_HASH_KECCAK256 / S2K_HASH_SHA3_256 (keccak.h).  digest_launch picks by alg.  They are not one kernel
// with a branch: its register allocation would be the larger of the two, and the sponge's 25-lane state is the larger.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "engine_internal.h"
#include "keccak.h"
#include "sha2.h"

namespace {

constexpr uint32_t DG_CAP = 256 * 64 + 64;   // bytes of LDS for a workgroup's stretch (s2k_debug_digest_caps)

// The workgroup's stretch msgs[lo, hi) into LDS; `base` = the 16-byte aligned address LDS byte 0 stands for.
__device__ __forceinline__ bool dg_stage(const uint8_t* __restrict__ msgs, uint64_t lo, uint64_t hi, uint8_t* lds, uintptr_t& base) {
  if (hi <= lo) return false;                              // (nothing to read: every item of the workgroup is empty)
  base = (uintptr_t)(msgs + lo) & ~(uintptr_t)15;
  const uint64_t bytes = (uint64_t)((uintptr_t)(msgs + hi) - base);
  if (bytes + 16 > DG_CAP) return false;
  for (uint32_t t = threadIdx.x * 16; t < (uint32_t)bytes; t += 256 * 16)
    *reinterpret_cast<uint4*>(lds + t) = *reinterpret_cast<const uint4*>(base + t);
  return true;
}

// NW big-endian words to o: 16-byte stores where the caller's output allows them, bytes otherwise
template <int NW>
__device__ __forceinline__ void dg_store(uint8_t* o, const uint32_t (&w)[NW], bool aligned) {
  if (aligned) {
#pragma unroll
    for (int k = 0; k < NW / 4; ++k)
      reinterpret_cast<uint4*>(o)[k] = make_uint4(__builtin_bswap32(w[4 * k]), __builtin_bswap32(w[4 * k + 1]), __builtin_bswap32(w[4 * k + 2]),
                                                  __builtin_bswap32(w[4 * k + 3]));
  } else {
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      o[4 * k] = (uint8_t)(w[k] >> 24);
      o[4 * k + 1] = (uint8_t)(w[k] >> 16);
      o[4 * k + 2] = (uint8_t)(w[k] >> 8);
      o[4 * k + 3] = (uint8_t)w[k];
    }
  }
}

// four little-endian lanes to o (a Keccak digest): the same choice of stores, no byte swap
__device__ __forceinline__ void dg_store_le(uint8_t* o, const uint64_t (&d)[4], bool aligned) {
  if (aligned) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
      reinterpret_cast<uint4*>(o)[k] = make_uint4((uint32_t)d[2 * k], (uint32_t)(d[2 * k] >> 32), (uint32_t)d[2 * k + 1], (uint32_t)(d[2 * k + 1] >> 32));
  } else {
#pragma unroll
    for (int k = 0; k < 32; ++k) o[k] = (uint8_t)(d[k / 8] >> (8 * (k % 8)));
  }
}

// What a lane of either digest kernel works on: its message (in LDS when the workgroup's stretch was staged, else in place),
// its output row, and whether the rows take 16-byte stores.  false: the lane has no item.  Every lane of the workgroup calls
// it (the staging ends in a barrier).
struct dg_item {
  const uint8_t* m;
  uint32_t len;
  uint8_t* o;
  bool aligned;
};
__device__ __forceinline__ bool dg_locate(dg_item& it, uint4* lds, uint32_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs,
                                          uint32_t msg_len, uint8_t* __restrict__ out, uint32_t out_stride) {
  const uint32_t b0 = blockIdx.x * 256;
  if (b0 >= n) return false;
  const uint32_t cnt = n - b0 < 256u ? n - b0 : 256u;
  const uint64_t lo = offs ? offs[b0] : (uint64_t)b0 * msg_len, hi = offs ? offs[b0 + cnt] : (uint64_t)(b0 + cnt) * msg_len;
  uintptr_t base = 0;
  const bool staged = dg_stage(msgs, lo, hi, reinterpret_cast<uint8_t*>(lds), base);
  __syncthreads();
  if (threadIdx.x >= cnt) return false;
  const uint32_t i = b0 + threadIdx.x;
  const uint64_t mo = offs ? offs[i] : (uint64_t)i * msg_len;
  it.len = offs ? (uint32_t)(offs[i + 1] - mo) : msg_len;
  it.m = staged ? reinterpret_cast<const uint8_t*>(lds) + ((uintptr_t)(msgs + mo) - base) : msgs + mo;
  it.o = out + (size_t)i * out_stride;
  it.aligned = (((uintptr_t)out | out_stride) & 15u) == 0;
  return true;
}

// out[i * out_stride .. + out_len) = the digest of message i: msgs[offs[i], offs[i + 1]), or msgs[i * msg_len, (i + 1) * msg_len)
// with offs null.  out_len is 32, or 64 (S2K_HASH_SHA512 only); bytes of a row behind out_len are not written.
__global__ void __launch_bounds__(256, 4)
k_digest_messages(uint32_t alg, uint32_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
                  uint8_t* __restrict__ out, uint32_t out_stride, uint32_t out_len) {
  __shared__ uint4 lds[DG_CAP / 16];
  dg_item it;
  if (!dg_locate(it, lds, n, msgs, offs, msg_len, out, out_stride)) return;
  const uint8_t* m = it.m;
  const uint32_t len = it.len;
  uint8_t* o = it.o;
  const bool aligned = it.aligned;
  if (alg == S2K_HASH_SHA512) {
    uint64_t st[8];
    s2k_sha2::sha512_message(st, m, len);
    if (out_len == 64) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        w[2 * k] = (uint32_t)(st[k] >> 32);
        w[2 * k + 1] = (uint32_t)st[k];
      }
      dg_store<16>(o, w, aligned);
    } else {                                               // the leftmost 32 bytes (hashToScalar, ecdsa.go:477-486)
      uint32_t w[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[2 * k] = (uint32_t)(st[k] >> 32);
        w[2 * k + 1] = (uint32_t)st[k];
      }
      dg_store<8>(o, w, aligned);
    }
  } else {
    uint32_t st[8];
    s2k_sha2::sha256_message(st, m, len);
    if (alg == S2K_HASH_SHA256D) s2k_sha2::sha256_again(st);
    dg_store<8>(o, st, aligned);
  }
}

// The same for S2K_HASH_KECCAK256 and S2K_HASH_SHA3_256 (out_len 32): the first four lanes of the sponge's state, little-endian.
__global__ void __launch_bounds__(256, 4)
k_digest_keccak(uint32_t alg, uint32_t n, const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint32_t msg_len,
                uint8_t* __restrict__ out, uint32_t out_stride) {
  __shared__ uint4 lds[DG_CAP / 16];
  dg_item it;
  if (!dg_locate(it, lds, n, msgs, offs, msg_len, out, out_stride)) return;
  uint64_t d[4];
  s2k_keccak::keccak256_message(d, it.m, it.len, alg == S2K_HASH_SHA3_256 ? s2k_keccak::DOMAIN_SHA3 : s2k_keccak::DOMAIN_KECCAK);
  dg_store_le(it.o, d, it.aligned);
}

inline bool alg_keccak(int alg) { return alg == S2K_HASH_KECCAK256 || alg == S2K_HASH_SHA3_256; }

int digest_launch(s2k_ctx* ctx, hipStream_t st, int alg, size_t n, const void* d_msgs, const void* d_offs, size_t msg_len, void* d_out,
                  size_t out_stride, size_t out_len) {
  if (alg_keccak(alg)) {
    k_digest_keccak<<<blocks_for(n), 256, 0, st>>>((uint32_t)alg, (uint32_t)n, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, (uint32_t)msg_len,
                                                   (uint8_t*)d_out, (uint32_t)out_stride);
    HIP_TRY(ctx, hipGetLastError());
    return S2K_OK;
  }
  k_digest_messages<<<blocks_for(n), 256, 0, st>>>((uint32_t)alg, (uint32_t)n, (const uint8_t*)d_msgs, (const uint64_t*)d_offs, (uint32_t)msg_len,
                                                   (uint8_t*)d_out, (uint32_t)out_stride, (uint32_t)out_len);
  HIP_TRY(ctx, hipGetLastError());
  return S2K_OK;
}

// What every form checks before anything is launched.  host: msgs / msg_offsets are the caller's host arrays - the offsets
// are scanned (a device form cannot: its precondition is s2k_schnorr_verify_batch_device's) and *total = the bytes to upload.
int msg_args(s2k_ctx* ctx, int alg, size_t n, const void* msgs, const uint64_t* msg_offsets, size_t msg_len, bool host, size_t* total) {
  if (alg != S2K_HASH_SHA256 && alg != S2K_HASH_SHA256D && alg != S2K_HASH_SHA512 && !alg_keccak(alg)) return fail(ctx, S2K_ERR_ARG, "unknown hash algorithm");
  if (msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "msg_len must be below 2^31");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  *total = 0;
  if (n == 0) return S2K_OK;
  if (!host) {
    if (!msgs && (msg_offsets || msg_len)) return fail(ctx, S2K_ERR_ARG, "null message buffer");
    return S2K_OK;
  }
  if (msg_offsets) {
    for (size_t i = 0; i < n; ++i) {
      if (msg_offsets[i + 1] < msg_offsets[i]) return fail(ctx, S2K_ERR_ARG, "msg_offsets decrease at item %zu", i);
      if (msg_offsets[i + 1] - msg_offsets[i] > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "message %zu is 2^31 bytes or longer", i);
    }
    *total = (size_t)msg_offsets[n];
  } else {
    *total = n * msg_len;                                  // (n < 2^30, msg_len < 2^31)
  }
  if (*total && !msgs) return fail(ctx, S2K_ERR_ARG, "null message buffer");
  return S2K_OK;
}

// The digests of a messages call into the context's buffer, on `st` behind whatever call of the context came before (that
// call may still be reading the buffer on another stream: ctx_enter).  The sibling that follows enters again, on the same
// stream, and leaves.
int digest_to_ctx(s2k_ctx* ctx, hipStream_t st, int alg, size_t n, const void* d_msgs, const void* d_offs, size_t msg_len, const uint8_t** dig) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = ctx_reserve(ctx, &ctx->msg_digest, &ctx->msg_digest_bytes, ((n + 255) & ~(size_t)255) * 32);
  if (rc) return rc;
  *dig = (const uint8_t*)ctx->msg_digest;
  return digest_launch(ctx, st, alg, n, d_msgs, d_offs, msg_len, ctx->msg_digest, 32, 32);
}

}  // namespace

// for the recovery calls that take messages (address.hip)
__attribute__((visibility("hidden"))) int s2k_internal_msg_args(s2k_ctx* ctx, int alg, size_t n, const void* msgs, const uint64_t* msg_offsets,
                                                                size_t msg_len, bool host, size_t* total) {
  return msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, host, total);
}
__attribute__((visibility("hidden"))) int s2k_internal_digest_to_ctx(s2k_ctx* ctx, hipStream_t st, int alg, size_t n, const void* d_msgs,
                                                                     const void* d_offs, size_t msg_len, const uint8_t** dig) {
  return digest_to_ctx(ctx, st, alg, n, d_msgs, d_offs, msg_len, dig);
}

extern "C" {

int s2k_debug_digest_caps(uint32_t out[1]) {
  if (!out) return S2K_ERR_ARG;
  out[0] = DG_CAP;
  return S2K_OK;
}

int s2k_digest_batch_device(s2k_ctx* ctx, int alg, size_t n, const void* d_msgs, const void* d_msg_offsets, size_t msg_len, void* d_out,
                            size_t out_len, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = msg_args(ctx, alg, n, d_msgs, (const uint64_t*)d_msg_offsets, msg_len, /*host=*/false, &total);
  if (rc) return rc;
  if (out_len != 32 && !(out_len == 64 && alg == S2K_HASH_SHA512)) return fail(ctx, S2K_ERR_ARG, "out_len must be 32, or 64 with S2K_HASH_SHA512");
  if (n == 0) return S2K_OK;
  if (!d_out) return fail(ctx, S2K_ERR_ARG, "null buffer");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return digest_launch(ctx, (hipStream_t)hip_stream, alg, n, d_msgs, d_msg_offsets, msg_len, d_out, out_len, out_len);
}

int s2k_digest_batch(s2k_ctx* ctx, int alg, size_t n, const uint8_t* msgs, const uint64_t* msg_offsets, size_t msg_len, uint8_t* out,
                     size_t out_len) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc) return rc;
  if (out_len != 32 && !(out_len == 64 && alg == S2K_HASH_SHA512)) return fail(ctx, S2K_ERR_ARG, "out_len must be 32, or 64 with S2K_HASH_SHA512");
  if (n == 0) return S2K_OK;
  if (!out) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const stage_part parts[3] = {part_msgs(msgs, total), part_offs(msg_offsets, n), stage_out(out, n * out_len)};
  return s2k_internal_staged_call(ctx, parts, 3, total + n * out_len, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_digest_batch_device(c, alg, n, d[0], msg_offsets ? d[1] : nullptr, msg_len, d[2], out_len, st);
  });
}

// Test hook: the kernel with an output stride of its own.  out[n * out_stride] goes up as the caller filled it and comes back
// whole, so the bytes between the rows show whether they were touched.  Synchronous; offsets scanned as in the host forms.
int s2k_debug_digest_strided(s2k_ctx* ctx, int alg, size_t n, const uint8_t* msgs, const uint64_t* msg_offsets, size_t msg_len, uint8_t* out,
                             size_t out_len, size_t out_stride) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc) return rc;
  if (out_len != 32 && !(out_len == 64 && alg == S2K_HASH_SHA512)) return fail(ctx, S2K_ERR_ARG, "out_len must be 32, or 64 with S2K_HASH_SHA512");
  if (out_stride < out_len || out_stride > 4096) return fail(ctx, S2K_ERR_ARG, "out_stride must be in out_len..4096");
  if (n == 0) return S2K_OK;
  if (!out) return fail(ctx, S2K_ERR_ARG, "null buffer");
  stage_part rows = stage_in(out, n * out_stride);
  rows.dst = out;                                          // up before the kernel, back after it
  const stage_part parts[3] = {part_msgs(msgs, total), part_offs(msg_offsets, n), rows};
  return s2k_internal_staged_call(ctx, parts, 3, 0, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return digest_launch(c, st, alg, n, d[0], msg_offsets ? d[1] : nullptr, msg_len, d[2], out_stride, out_len);
  });
}

// ---- ECDSA verification from messages: digests into the context's buffer, then the digest sibling on the same stream ----
// Every form first gives its sibling a call of zero items, which runs the sibling's checks of the context, the key set and
// the flags and launches nothing: a refused call has launched nothing, the digest kernel included.

int s2k_ecdsa_verify_messages_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub_xy, int alg, const void* d_msgs, const void* d_msg_offsets,
                                           size_t msg_len, const void* d_r, const void* d_s, uint32_t flags, void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = msg_args(ctx, alg, n, d_msgs, (const uint64_t*)d_msg_offsets, msg_len, /*host=*/false, &total);
  if (rc || n == 0) return rc;
  if (!d_pub_xy || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const uint8_t* dig = nullptr;
  rc = digest_to_ctx(ctx, (hipStream_t)hip_stream, alg, n, d_msgs, d_msg_offsets, msg_len, &dig);
  if (rc) return rc;
  return s2k_ecdsa_verify_batch_device(ctx, n, d_pub_xy, dig, d_r, d_s, flags, d_valid, hip_stream);
}

int s2k_ecdsa_verify_messages_batch(s2k_ctx* ctx, size_t n, const uint8_t* pub, int alg, const uint8_t* msgs, const uint64_t* msg_offsets,
                                    size_t msg_len, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc || n == 0) return rc;
  if (!pub || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  // (the small-call route of s2k_ecdsa_verify_batch: the page-locked block, no DMA transfers)
  const bool small = s2k_internal_small_call(ctx, n, flags) && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF) && total <= DG_SMALL_BYTES;
  const stage_part parts[6] = {stage_in(pub, n * 64), part_msgs(msgs, total), part_offs(msg_offsets, n), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 6, n * 128 + total, small, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_messages_batch_device(c, n, d[0], alg, d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], d[4], flags, d[5], st);
  });
}

// The ticket form (s2k_wait): messages, offsets, keys and signatures cross on the copy stream beside the kernels of the tickets
// before it; all of them must stay alive until the ticket has been waited for.
int s2k_ecdsa_verify_messages_batch_submit(s2k_ctx* ctx, size_t n, const uint8_t* pub, int alg, const uint8_t* msgs, const uint64_t* msg_offsets,
                                           size_t msg_len, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* valid, s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  size_t total = 0;
  int rc = msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc) return rc;
  if (n && (!pub || !r || !s || !valid)) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const stage_part parts[6] = {stage_in(pub, n * 64), part_msgs(msgs, total), part_offs(msg_offsets, n), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_submit(ctx, n, valid, parts, 6, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_messages_batch_device(c, n, d[0], alg, d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], d[4], flags, d[5], st);
  }, ticket);
}

int s2k_ecdsa_verify_messages_batch_keyset_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_key_index, int alg, const void* d_msgs,
                                                  const void* d_msg_offsets, size_t msg_len, const void* d_r, const void* d_s, uint32_t flags,
                                                  void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = s2k_ecdsa_verify_batch_keyset_device(ctx, ks, 0, nullptr, nullptr, nullptr, nullptr, flags, nullptr, hip_stream);
  if (rc) return rc;
  size_t total = 0;
  rc = msg_args(ctx, alg, n, d_msgs, (const uint64_t*)d_msg_offsets, msg_len, /*host=*/false, &total);
  if (rc || n == 0) return rc;
  if (!d_key_index || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (flags & S2K_ECDSA_FORCE_COMPLETE) return fail(ctx, S2K_ERR_ARG, "S2K_ECDSA_FORCE_COMPLETE does not apply to key sets");
  const uint8_t* dig = nullptr;
  rc = digest_to_ctx(ctx, (hipStream_t)hip_stream, alg, n, d_msgs, d_msg_offsets, msg_len, &dig);
  if (rc) return rc;
  return s2k_ecdsa_verify_batch_keyset_device(ctx, ks, n, d_key_index, dig, d_r, d_s, flags, d_valid, hip_stream);
}

int s2k_ecdsa_verify_messages_batch_keyset(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* key_index, int alg, const uint8_t* msgs,
                                           const uint64_t* msg_offsets, size_t msg_len, const uint8_t* r, const uint8_t* s, uint32_t flags,
                                           uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = s2k_ecdsa_verify_batch_keyset_device(ctx, ks, 0, nullptr, nullptr, nullptr, nullptr, flags, nullptr, nullptr);
  if (rc) return rc;
  size_t total = 0;
  rc = msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc || n == 0) return rc;
  if (!key_index || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (flags & S2K_ECDSA_FORCE_COMPLETE) return fail(ctx, S2K_ERR_ARG, "S2K_ECDSA_FORCE_COMPLETE does not apply to key sets");
  const bool small = s2k_internal_small_call(ctx, n, flags) && total <= DG_SMALL_BYTES;
  const stage_part parts[6] = {stage_in(key_index, n * 4), part_msgs(msgs, total), part_offs(msg_offsets, n), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 6, n * 68 + total, small, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_messages_batch_keyset_device(c, ks, n, d[0], alg, d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], d[4], flags, d[5], st);
  });
}

int s2k_ecdsa_verify_messages_batch_keyset_bykey_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_pub_xy, int alg, const void* d_msgs,
                                                        const void* d_msg_offsets, size_t msg_len, const void* d_r, const void* d_s, uint32_t flags,
                                                        void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = s2k_ecdsa_verify_batch_keyset_bykey_device(ctx, ks, 0, nullptr, nullptr, nullptr, nullptr, flags, nullptr, hip_stream);
  if (rc) return rc;
  size_t total = 0;
  rc = msg_args(ctx, alg, n, d_msgs, (const uint64_t*)d_msg_offsets, msg_len, /*host=*/false, &total);
  if (rc || n == 0) return rc;
  if (!d_pub_xy || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const uint8_t* dig = nullptr;
  rc = digest_to_ctx(ctx, (hipStream_t)hip_stream, alg, n, d_msgs, d_msg_offsets, msg_len, &dig);
  if (rc) return rc;
  return s2k_ecdsa_verify_batch_keyset_bykey_device(ctx, ks, n, d_pub_xy, dig, d_r, d_s, flags, d_valid, hip_stream);
}

int s2k_ecdsa_verify_messages_batch_keyset_bykey(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint8_t* pub, int alg, const uint8_t* msgs,
                                                 const uint64_t* msg_offsets, size_t msg_len, const uint8_t* r, const uint8_t* s, uint32_t flags,
                                                 uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = s2k_ecdsa_verify_batch_keyset_bykey_device(ctx, ks, 0, nullptr, nullptr, nullptr, nullptr, flags, nullptr, nullptr);
  if (rc) return rc;
  size_t total = 0;
  rc = msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc || n == 0) return rc;
  if (!pub || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  // (a batch the plain call would verify on its wave-per-signature or four-lanes-per-signature ladder IS the plain call, as in
  // s2k_ecdsa_verify_batch_keyset_bykey - with its small-call route)
  if (s2k_internal_bykey_delegates(ctx, n, flags)) return s2k_ecdsa_verify_messages_batch(ctx, n, pub, alg, msgs, msg_offsets, msg_len, r, s, flags, valid);
  const stage_part parts[6] = {stage_in(pub, n * 64), part_msgs(msgs, total), part_offs(msg_offsets, n), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 6, n * 128 + total, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_messages_batch_keyset_bykey_device(c, ks, n, d[0], alg, d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], d[4], flags, d[5], st);
  });
}

}  // extern "C"
