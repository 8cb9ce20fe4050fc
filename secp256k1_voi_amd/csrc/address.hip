// address.hip — Keccak-256 addresses on the device: of 65-byte key records (s2k_keccak_address_batch) and of the keys recovered
// from signatures (s2k_ecdsa_recover_address_batch, and its form that takes messages).  The callers who recover keys in bulk
// want addr = Keccak-256(X || Y)[12..32), not the key; hashed here, 20 bytes per item go back instead of 65 and no per-item
// work is left on the host.
//
// One kernel serves every place that writes key records (k_affine_finish<MODE_RECOVER>, the worklist, the fallback,
// k_recover_row): the recovery call runs unchanged into a buffer of the context (s2k_ctx::rec_keys, 65 bytes per item), and
// k_keccak_address runs behind it on the same stream.  One lane per record, 256 per workgroup.  A record's key bytes start
// at 65 i + 1 and the 20-byte rows at 20 i of a caller's device buffer, so neither is ever aligned: the workgroup's 256 x 65
// contiguous bytes come through LDS with aligned 16-byte loads (the rule of dg_stage, digest.hip: an aligned load that holds
// one byte of the stretch never leaves that byte's page), and its 256 x 20 contiguous bytes of rows leave through LDS as
// dwords, or as bytes when the caller's rows are not 4-byte aligned.  Exactly 20 n bytes are written.  Public data only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "engine_internal.h"
#include "keccak.h"

namespace {

constexpr uint32_t AD_LDS = 256 * 65 + 32;   // a workgroup's records, and up to 15 bytes in front of them, in 16-byte pieces

__global__ void __launch_bounds__(256, 4)
k_keccak_address(uint32_t n, const uint8_t* __restrict__ pub65, const uint8_t* __restrict__ ok, uint8_t* __restrict__ addr20) {
  __shared__ uint4 lds[AD_LDS / 16];
  uint8_t* l8 = reinterpret_cast<uint8_t*>(lds);
  uint32_t* l32 = reinterpret_cast<uint32_t*>(lds);
  const uint32_t b0 = blockIdx.x * 256;
  if (b0 >= n) return;
  const uint32_t cnt = n - b0 < 256u ? n - b0 : 256u;
  const uint8_t* lo = pub65 + (size_t)b0 * 65;
  const uintptr_t base = (uintptr_t)lo & ~(uintptr_t)15;
  const uint32_t lead = (uint32_t)((uintptr_t)lo - base), bytes = lead + cnt * 65;      // bytes <= 15 + 16640 < AD_LDS - 16
  for (uint32_t t = threadIdx.x * 16; t < bytes; t += 256 * 16) *reinterpret_cast<uint4*>(l8 + t) = *reinterpret_cast<const uint4*>(base + t);
  __syncthreads();
  const bool have = threadIdx.x < cnt;
  uint32_t w[5] = {0, 0, 0, 0, 0};                        // the row: 20 zero bytes unless the record is a key
  if (have) {
    const uint8_t* rec = l8 + lead + threadIdx.x * 65;
    if (rec[0] == 0x04 && (!ok || ok[b0 + threadIdx.x])) {
      uint64_t d[4];
      s2k_keccak::keccak256_64(d, rec + 1);
      w[0] = (uint32_t)(d[1] >> 32);                      // digest bytes 12..32: the lanes are little-endian, and so are the dwords
      w[1] = (uint32_t)d[2];
      w[2] = (uint32_t)(d[2] >> 32);
      w[3] = (uint32_t)d[3];
      w[4] = (uint32_t)(d[3] >> 32);
    }
  }
  __syncthreads();                                        // every record has been read: the block becomes the rows
  if (have) {
#pragma unroll
    for (int k = 0; k < 5; ++k) l32[threadIdx.x * 5 + k] = w[k];
  }
  __syncthreads();
  uint8_t* dst = addr20 + (size_t)b0 * 20;
  if (((uintptr_t)dst & 3u) == 0) {
    for (uint32_t t = threadIdx.x; t < cnt * 5; t += 256) reinterpret_cast<uint32_t*>(dst)[t] = l32[t];
  } else {
    for (uint32_t t = threadIdx.x; t < cnt * 20; t += 256) dst[t] = l8[t];
  }
}

// the addresses of n records behind whatever the context enqueued before on `st`
int address_launch(s2k_ctx* ctx, hipStream_t st, size_t n, const void* d_pub65, const void* d_ok, void* d_addr20) {
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  k_keccak_address<<<blocks_for(n), 256, 0, st>>>((uint32_t)n, (const uint8_t*)d_pub65, (const uint8_t*)d_ok, (uint8_t*)d_addr20);
  HIP_TRY(ctx, hipGetLastError());
  return ctx_leave(ctx, st);
}

// s2k_ecdsa_recover_batch_device, unchanged, into the context's buffer of key records, and their addresses behind it
int recover_then_address(s2k_ctx* ctx, hipStream_t st, size_t n, const void* d_dig, const void* d_r, const void* d_s, const void* d_recid,
                         uint32_t flags, void* d_addr20, void* d_ok) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_enter(ctx, st);                            // (the call before may still read the buffer on another stream)
  if (rc) return rc;
  rc = ctx_reserve(ctx, &ctx->rec_keys, &ctx->rec_keys_bytes, ((n + 255) & ~(size_t)255) * 65);
  if (rc) return rc;
  rc = s2k_ecdsa_recover_batch_device(ctx, n, d_dig, d_r, d_s, d_recid, flags, ctx->rec_keys, d_ok, st);
  if (rc) return rc;
  return address_launch(ctx, st, n, ctx->rec_keys, d_ok, d_addr20);
}

}  // namespace

extern "C" {

int s2k_keccak_address_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub65, const void* d_ok, void* d_addr20, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_pub65 || !d_addr20) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  return address_launch(ctx, (hipStream_t)hip_stream, n, d_pub65, d_ok, d_addr20);
}

int s2k_keccak_address_batch(s2k_ctx* ctx, size_t n, const uint8_t* pub65, const uint8_t* ok, uint8_t* addr20) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!pub65 || !addr20) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  const stage_part parts[3] = {stage_in(pub65, n * 65), stage_in(ok, ok ? n : 0, ok ? n : 8), stage_out(addr20, n * 20)};
  return s2k_internal_staged_call(ctx, parts, 3, n * 85, s2k_internal_small_call(ctx, n, 0u), [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_keccak_address_batch_device(c, n, d[0], ok ? d[1] : nullptr, d[2], st);
  });
}

int s2k_ecdsa_recover_address_batch_device(s2k_ctx* ctx, size_t n, const void* d_dig, const void* d_r, const void* d_s, const void* d_recid,
                                           uint32_t flags, void* d_addr20, void* d_ok, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_dig || !d_r || !d_s || !d_recid || !d_addr20 || !d_ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  return recover_then_address(ctx, (hipStream_t)hip_stream, n, d_dig, d_r, d_s, d_recid, flags, d_addr20, d_ok);
}

int s2k_ecdsa_recover_address_batch(s2k_ctx* ctx, size_t n, const uint8_t* dig, const uint8_t* r, const uint8_t* s, const uint8_t* recid,
                                    uint32_t flags, uint8_t* addr20, uint8_t* ok) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!dig || !r || !s || !recid || !addr20 || !ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  const stage_part parts[6] = {stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_in(recid, n), stage_out(addr20, n * 20), stage_out(ok, n)};
  return s2k_internal_staged_call(ctx, parts, 6, n * 97, s2k_internal_small_call(ctx, n, flags), [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_recover_address_batch_device(c, n, d[0], d[1], d[2], d[3], flags, d[4], d[5], st);
  });
}

// The messages forms: the digest kernel in front, into the context's digest buffer (digest.hip).
int s2k_ecdsa_recover_address_messages_batch_device(s2k_ctx* ctx, size_t n, int alg, const void* d_msgs, const void* d_msg_offsets, size_t msg_len,
                                                    const void* d_r, const void* d_s, const void* d_recid, uint32_t flags, void* d_addr20,
                                                    void* d_ok, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = s2k_internal_msg_args(ctx, alg, n, d_msgs, (const uint64_t*)d_msg_offsets, msg_len, /*host=*/false, &total);
  if (rc || n == 0) return rc;
  if (!d_r || !d_s || !d_recid || !d_addr20 || !d_ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const uint8_t* dig = nullptr;
  rc = s2k_internal_digest_to_ctx(ctx, (hipStream_t)hip_stream, alg, n, d_msgs, d_msg_offsets, msg_len, &dig);
  if (rc) return rc;
  return recover_then_address(ctx, (hipStream_t)hip_stream, n, dig, d_r, d_s, d_recid, flags, d_addr20, d_ok);
}

int s2k_ecdsa_recover_address_messages_batch(s2k_ctx* ctx, size_t n, int alg, const uint8_t* msgs, const uint64_t* msg_offsets, size_t msg_len,
                                             const uint8_t* r, const uint8_t* s, const uint8_t* recid, uint32_t flags, uint8_t* addr20,
                                             uint8_t* ok) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  size_t total = 0;
  int rc = s2k_internal_msg_args(ctx, alg, n, msgs, msg_offsets, msg_len, /*host=*/true, &total);
  if (rc || n == 0) return rc;
  if (!r || !s || !recid || !addr20 || !ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const bool small = s2k_internal_small_call(ctx, n, flags) && total <= DG_SMALL_BYTES;
  const stage_part parts[7] = {part_msgs(msgs, total), part_offs(msg_offsets, n), stage_in(r, n * 32), stage_in(s, n * 32),
                               stage_in(recid, n),     stage_out(addr20, n * 20), stage_out(ok, n)};
  return s2k_internal_staged_call(ctx, parts, 7, n * 65 + total, small, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_recover_address_messages_batch_device(c, n, alg, d[0], msg_offsets ? d[1] : nullptr, msg_len, d[2], d[3], d[4], flags, d[5], d[6], st);
  });
}

}  // extern "C"
