// engine_internal.h — pieces shared by the translation units of the engine (engine.hip, gtable.hip, keyed.hip, msm.hip ...).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>

#include "../../include/secp256k1_voi_amd.h"
#include "fe.h"
#include "point.h"

using namespace s2k;

// Most per-key tables a verification call builds (10 KiB each: 40 GiB at the cap; the buffer is sized by the batch,
// n / min_group tables, so a 2^20 batch holds 2.4 GB whatever this says).  Was 2^18 until the end of round 3: a batch of
// 2^24 signatures of 2^20 keys then built no tables at all (threshold raised to 64 per key) and took 129 ms instead of 80.
constexpr uint32_t KG_MAX_TABLES_DEFAULT = 1u << 22;

// ---- generator tables (layout, registry and background build: gtable.hip) ----
// The window width is a RUNTIME property of a table since round 5: a context starts on a narrow table
// that is built while it is created (S2K_GT_BITS_FIRST: 20 bits, 0.8 GiB, < 0.1 s) and moves to the wide one when a background
// thread has built it (S2K_GT_BITS: the width an automatic context aims for when the device has the memory; else 24, else 22).
// Same-box A/B on MI355X, ms per 2^20 verifications / table size / time to build: round 3, ungrouped flow (tools/ab_gtbits.sh)
// 16 bits 9.21 / 64 MiB / 0.05 s, 20 bits 9.10 / 0.8 GiB, 22 bits 9.04 / 3 GiB / 0.3 s, 24 bits 9.03 / 11 GiB / 0.9 s; end of
// round 4, grouped flow (tools/gpu_gtbits_keyset.sh): 22 / 24 / 26 bits 4.95-4.97 / 4.97 / 4.85-4.87 ms, key set with 5-bit
// joint tables 2.46-2.47 / 2.42 / 2.41-2.42 ms.  26 bits are TEN windows (nine would take 29 bits and 309 GB): 40 GiB per device,
// shared by the contexts of a process, 3.1 s to build - which no caller waits for any more.
#ifndef S2K_GT_BITS
#define S2K_GT_BITS 26
#endif
#ifndef S2K_GT_BITS_FIRST
#define S2K_GT_BITS_FIRST 20
#endif
constexpr int GT_BITS_TARGET = S2K_GT_BITS, GT_BITS_FIRST = S2K_GT_BITS_FIRST, GT_BITS_MIN = 8, GT_BITS_MAX = 26;
static_assert(GT_BITS_TARGET >= GT_BITS_MIN && GT_BITS_TARGET <= GT_BITS_MAX, "generator window width out of range");   // (26 bits: 10 windows, 43 GB)
static_assert(GT_BITS_FIRST >= GT_BITS_MIN && GT_BITS_FIRST <= GT_BITS_MAX, "first generator window width out of range");
inline constexpr uint32_t gt_windows_of(int bits) { return (uint32_t)((256 + bits - 1) / bits); }
inline constexpr size_t gt_entries_of(int bits) { return (size_t)gt_windows_of(bits) << bits; }
inline constexpr size_t gt_bytes_of(int bits) { return gt_entries_of(bits) * 64; }

// what a kernel gets: the table and its geometry, by value.  A CALL uses one view for all its launches (s2k_ctx::gt_call,
// loaded by ctx_enter): the ladder kernels leave lanes for the worklist kernel whose tags name an entry of the table they ran
// on (WL_DOUBLE_LAST, verify_fast.h and worklist.hip), so the background build may publish the wide table between two calls, never inside one.
struct gt_view {
  const uint32_t* p;
  uint32_t bits, windows;
};

S2K_DEV apt gt_load(const gt_view& gt, uint32_t window, uint32_t digit) {
  const uint4* p = reinterpret_cast<const uint4*>(gt.p + ((((size_t)window << gt.bits) | digit) << 4));
  uint4 a = p[0], b = p[1], c = p[2], d = p[3];
  apt r;
  r.x.v[0] = a.x; r.x.v[1] = a.y; r.x.v[2] = a.z; r.x.v[3] = a.w;
  r.x.v[4] = b.x; r.x.v[5] = b.y; r.x.v[6] = b.z; r.x.v[7] = b.w;
  r.y.v[0] = c.x; r.y.v[1] = c.y; r.y.v[2] = c.z; r.y.v[3] = c.w;
  r.y.v[4] = d.x; r.y.v[5] = d.y; r.y.v[6] = d.z; r.y.v[7] = d.w;
  return r;
}
// next digit (`bits` wide, 8 .. 26) of a 256-bit scalar held in u[0..7] (consumed from the bottom)
S2K_DEV uint32_t gt_next_digit(uint32_t u[8], uint32_t bits) {
  uint32_t d = u[0] & ((1u << bits) - 1u);
#pragma unroll
  for (int i = 0; i < 7; ++i) u[i] = (u[i] >> bits) | (u[i + 1] << (32u - bits));
  u[7] >>= bits;
  return d;
}

// big-endian 32-byte strings at arbitrary alignment (65-byte point records)
S2K_DEV void load_be32_unaligned(uint32_t out[8], const uint8_t* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint8_t* q = p + (7 - i) * 4;
    out[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
}
S2K_DEV void store_be32_unaligned(uint8_t* p, const uint32_t in[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint8_t* q = p + (7 - i) * 4;
    q[0] = (uint8_t)(in[i] >> 24); q[1] = (uint8_t)(in[i] >> 16); q[2] = (uint8_t)(in[i] >> 8); q[3] = (uint8_t)in[i];
  }
}

// Largest batch the wave-per-signature ladders (k_verify_row / k_schnorr_row / k_recover_row, small_call.hip) take: above it the
// lane-per-signature kernels win (profiles/r05_small_batch_ab.txt, ECDSA: 0.19 against 0.68 ms up to 1024 signatures - one wave
// per SIMD -, 0.41 against 0.7-1.1 at 4096, 0.71 against 1.08 at 8192, 1.31 against 1.10 at 16384 device-resident; from host
// memory 0.28 against 0.74 ms at 1024, 0.50 against 0.75 at 4096, 0.77 against 0.78 at 8192).
// Largest batch the four-lanes-per-signature ladder (k_verify_quad) takes, above the row kernels' threshold
// (profiles/r05_mid_batch_ab.txt: 0.35 ms for anything from 2^11 to 2^14 signatures - one wave per SIMD at 2^14 -, 0.61 at 2^15,
// 1.10 at 2^16; the lane kernels 0.59-0.72 over that range, the row kernels 0.26 at 2^11 and 0.42 at 2^12).
#ifndef S2K_QUAD_MAX_DEFAULT
#define S2K_QUAD_MAX_DEFAULT 32768
#endif
#ifndef S2K_ROW_MAX_DEFAULT
#define S2K_ROW_MAX_DEFAULT 3072
#endif
// Largest key-set call the wave-per-signature ladder over the set's tables takes (k_verify_row_keyset / k_schnorr_row_keyset;
// s2k_ctx_set_keyset_small_batch_max): the largest measured size at which it beats the lane-per-signature key-set path by
// more than that path's own spread in both algorithms (profiles/r14_keyset_row_time.jsonl, device-resident, a JOINT5 set of
// 1024 keys: ECDSA 0.14 against 0.28 ms up to 1024 signatures, 0.19 against 0.29 at 2048, 0.24 against 0.28 at 3072, 0.32
// against 0.29 at 4096; BIP-340 0.10 against 0.33-0.39 up to 1024, 0.20 against 0.39 at 2048, 0.29 against 0.33 at 3072 - inside
// that path's spread of 0.06 -, 0.39 against 0.33 at 4096)
#ifndef S2K_KS_ROW_MAX_DEFAULT
#define S2K_KS_ROW_MAX_DEFAULT 2048
#endif

// ---- host side ----
struct s2k_ctx {
  int device = -1;
  bool gt_held = false;         // this context holds a reference on its device's generator tables (gtable_acquire)
  int gt_fixed = 0;             // s2k_ctx_create_ex with an explicit width: only the table of that width is used (0: the widest ready)
  gt_view gt_call = {nullptr, 0, 0};   // the generator table of the call being enqueued: loaded ONCE per call (ctx_enter), passed to every launch of it
  int dbg_gt_swap = 0;          // test hook (s2k_debug_gt_swap_in_call): publish this width between the ladder and the worklist launch of the next call
  char gt_note[200] = {0};      // s2k_ctx_gt_note's answer (copied under the registry's lock)
  void* ws = nullptr;           // workspace of the verification path
  size_t ws_bytes = 0;
  void* msm_ws = nullptr;       // workspace of the multi-scalar multiplication
  size_t msm_ws_bytes = 0;
  void* seg_ws = nullptr;       // workspace of the segmented multi-scalar multiplication (msm_seg.hip), allocated on its first call
  size_t seg_ws_bytes = 0;
  void* seg_host = nullptr;     // pinned host block its plan is uploaded from (one copy per call)
  size_t seg_host_bytes = 0;
  void* h2c_dev = nullptr;      // hashing to the curve (h2c.hip): status word and DST_prime on the device, allocated on its first call
  void* h2c_host = nullptr;     // ... and the pinned host block both travel through
  void* msg_digest = nullptr;   // the verification calls that take messages (digest.hip): 32 bytes per item, what k_digest_messages
  size_t msg_digest_bytes = 0;  // writes and the digest call behind it reads; allocated on the first such call
  void* rec_keys = nullptr;     // the recovery calls that return addresses (address.hip): 65 bytes per item, the key records
  size_t rec_keys_bytes = 0;    // s2k_ecdsa_recover_batch_device writes and k_keccak_address reads; allocated on the first such call
  void* rlc_save = nullptr;     // kept terms of a rejected whole-batch check (BIP-340, recoverable ECDSA) while its failing
                                // signatures are located; the ECDSA leaf verifier's recovered keys
  size_t rlc_save_bytes = 0;
  // host-buffer entry point: device staging for inputs / verdicts, a copy stream and a compute
  // stream, events that chain them (created on first use)
  void* io = nullptr;
  size_t io_bytes = 0;
  // small synchronous host calls (s2k_internal_small_block, pipeline.hip): a page-locked block the kernels read and write in place
  uint8_t* h_small = nullptr;
  uint8_t* d_small = nullptr;   // the same block as the device addresses it
  size_t h_small_bytes = 0;
  hipStream_t s_copy = nullptr, s_comp = nullptr;
  // A child context of submit / wait owns buffers, not streams: its copy stream is its parent's, its two compute streams
  // those of its LANE (even tickets: the parent's own; odd tickets: a second pair).  Within a lane tickets run their kernels
  // strictly one after the other, each with the two-stream overlap of a resident call; the two lanes run beside each other
  // like two contexts (worth 3 %), and the transfers run ahead of both (also for what was tried
  // before: a stream set per ticket - the front ends crawl beside three ladders, empty tail launches of 161 VGPRs wait
  // milliseconds for room, and streams beyond the hardware queues serialise at random).
  bool streams_shared = false;
  hipEvent_t ev_copied[2] = {nullptr, nullptr};
  hipEvent_t ev_arrival[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // pieces of a pinned batch on their way in
  int cu_count = 0;
  // Calls on one context share its workspaces.  Every enqueue ends by recording ev_done on its
  // stream, and an enqueue on a different stream than the previous one first waits for it, so
  // consecutive calls never overlap on the device whatever streams they use.
  hipEvent_t ev_done = nullptr;
  hipStream_t last_stream = nullptr;
  bool have_last = false;
  // optional per-kernel timing of the verification path (s2k_ctx_profile): event quadruples
  // around k_scalar_prep / k_verify_fast / k_verify_fallback, read back by s2k_ctx_profile_read
  bool prof_on = false;
  hipEvent_t* prof_ev = nullptr;
  size_t prof_cap = 0, prof_used = 0;
  uint64_t* clk = nullptr;      // device: s_memtime / s_memrealtime stamps of one wave of k_verify_fast
  // the same for the multi-scalar path (s2k_ctx_profile_msm): MSM_PROF_EV events per call, see msm_prof_mark
  hipEvent_t* msm_prof_ev = nullptr;
  size_t msm_prof_cap = 0, msm_prof_used = 0;
  bool msm_prof_on = false;
  // repeated-key path (keyed.hip): grouping arrays and per-key tables, grown on demand
  uint32_t quad_max = S2K_QUAD_MAX_DEFAULT;   // ... and up to this many the four-lanes-per-signature ladder (s2k_ctx_set_mid_batch_max)
  uint32_t row_max = S2K_ROW_MAX_DEFAULT;   // batches of up to this many signatures take the wave-per-signature ladder (s2k_ctx_set_small_batch_max)
  uint32_t ks_row_max = S2K_KS_ROW_MAX_DEFAULT;   // key-set calls of up to this many signatures take the row ladder over the set's tables (s2k_ctx_set_keyset_small_batch_max)
  uint32_t ks_comb_row_max = 0;      // ... and those over a COMB set of up to this many k_verify_row_comb / k_schnorr_row_comb (s2k_ctx_set_keyset_comb_small_batch_max; 0: never)
  int ks_last = -1;                  // S2K_KEYSET_LADDER_* of the last key-set verification call (-1: none yet)
  int kg_mode = S2K_KEYS_ADAPTIVE;
  uint32_t kg_min_group = 0, kg_hash_bits = 0, kg_max_tables = KG_MAX_TABLES_DEFAULT;
  uint32_t kg_table_cap = 0;         // 0: none; else the table count the device had memory for (s2k_internal_key_reserve)
  uint64_t kg_seed = 0;              // hash seed of the key grouping (operating-system randomness, per context)
  hipStream_t s_aux = nullptr;       // scalar preparation runs here, beside the grouping and the table kernels
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mid = nullptr, ev_part0 = nullptr, ev_part1 = nullptr;
  hipStream_t s_aux2 = nullptr;      // two-part flow: the second half of the tables is built here, beside the first half's ladder
  hipStream_t s_msm_tail = nullptr;  // multi-scalar multiplication in two parts (msm.hip): the upper windows' tail, beside the lower windows' bucket pass
  uint32_t kg_parts = 1;             // 1: all tables, then all ladders; 2: the two-part flow (S2K_KEYED_PARTS; measured slower)
  uint32_t gp_first_percent = 60;    // share of k_generator_part launched beside k_key_chain (the rest: beside k_key_finish)
  // ECDSA and BIP-340 verification calls build their per-key tables as a comb (kc_geom below) unless the window path is asked
  // for (s2k_ctx_set_keyed_ladder; S2K_KEYED_LADDER=window when the context is created); kt_comb_call: what the call being
  // enqueued uses (the verification entry points set it around grouped_front, s2k_internal_key_group reads it)
  bool kt_comb = true, kt_comb_call = false;
  int kt_last = -1;                  // S2K_LADDER_* of the last ECDSA or BIP-340 verification call's tables (-1: it built none)
  void* kg = nullptr;
  size_t kg_bytes = 0;
  void* ktab = nullptr;
  size_t ktab_bytes = 0;
  void* xkeys = nullptr;             // BIP-340 over a key set: the x-only keys of a call's signatures, expanded from the set
  size_t xkeys_bytes = 0;
  void* ks_found = nullptr;          // ECDSA over a key set by key bytes: the key indices the set's index found for a call's signatures
  size_t ks_found_bytes = 0;
  // encoded ECDSA over a key set (ingest.hip): device counters of the last synchronous call (EK_* below; allocated on the
  // first such call), the items of its pieces the set was not used for, and whether there was such a call at all
  uint32_t* ek_ctr = nullptr;
  uint64_t ek_delegated = 0;
  bool ek_have = false;
  uint32_t* kg_counters = nullptr;   // device, KG_COUNTERS words (of the last call; null: it did not group)
  uint32_t kg_last_max_tables = 0;   // table cap of that call (the device counter of tables is not clamped)
  uint32_t* last_wl_count = nullptr; // device: the last verification call's complete-formula worklist length
  // S2K_KEYS_ADAPTIVE (the default): what the grouping of recent calls found, learned WITHOUT synchronising.  k_key_counts of
  // a grouped call stores (sequence number << 32 | signatures that got a table) into a slot of `kga_note` (page-locked host
  // memory, eight slots); the next calls read the slots that have arrived.  After KG_ADAPT_MISSES consecutive observed
  // batches (of at least KG_ADAPT_MIN_BATCH signatures) in which no key reached the threshold, the next KG_ADAPT_SKIP such
  // batches are verified without looking (the general ladder, exactly as S2K_KEYS_OFF), then one batch looks again; the first
  // observed batch that does find a group ends the skipping.  Children of submit / wait use their parent's state (parent).
  s2k_ctx* parent = nullptr;                // of a child context of submit / wait (else null)
  unsigned long long* kga_note = nullptr;   // host, page-locked, KG_ADAPT_SLOTS entries
  uint32_t kga_seq = 0;                     // sequence number of the last grouped call that was asked to leave a note
  uint32_t kga_seen = 0;                    // ... of the last note taken into account
  uint32_t kga_miss_streak = 0, kga_skip_left = 0;
  bool kga_skipping = false;
  uint32_t kga_skipped = 0, kga_probes = 0, kga_observed = 0;   // totals (s2k_ctx_key_grouping_adaptive)
  unsigned long long* kg_note_dst = nullptr;   // where THIS call's k_key_counts leaves its note (null: nowhere), and its number
  uint32_t kg_note_seq = 0;
  // submit / wait (s2k_ecdsa_verify_batch_submit, s2k_wait): child contexts on the same device take the submitted
  // batches in turn, so that one batch's transfer, grouping and tables run beside another's ladder.  A child owns
  // its own workspaces, staging and streams (the generator tables are shared per device); `pipe` is empty in a child.
  struct pipe_slot {
    s2k_ctx* ctx = nullptr;        // the child context (created on first use)
    uint64_t ticket = 0;           // ticket in flight on it (0: none)
    uint8_t* dst = nullptr;        // where its verdicts go (the caller's array)
    size_t n = 0;
    hipEvent_t done = nullptr;     // recorded behind the ticket's last operation (the verdicts' copy out)
    uint8_t* h_valid = nullptr;    // page-locked landing buffer of the verdicts (when dst is pageable)
    size_t h_valid_bytes = 0;
    bool direct = false;           // dst is page-locked itself: the device-to-host copy lands there
    hipEvent_t t_begin = nullptr, t_copied = nullptr, t_end = nullptr;   // s2k_ctx_ticket_timing: before / behind the ticket's host-to-device copies, behind its verdicts
    bool timed = false;            // the three events were recorded for the ticket in flight
  };
  static constexpr unsigned PIPE_SLOTS = 4;   // batches in flight: two LANES (even and odd tickets), each with one batch
                                              // computing and one arriving
  pipe_slot pipe[PIPE_SLOTS];
  hipStream_t lane1_comp = nullptr, lane1_aux = nullptr;   // the compute streams of the odd tickets (the even ones: s_comp, s_aux)
  uint64_t pipe_next = 1;          // next ticket (ticket t runs on slot t mod PIPE_SLOTS)
  uint64_t pipe_failed[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // tickets retired with an error (by a later submit), and their codes
  int pipe_failed_rc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned pipe_failed_n = 0;
  bool pipe_timing = false;        // s2k_ctx_ticket_timing
  uint64_t pipe_times_ticket[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the last retired tickets and their times (s2k_ticket_times)
  float pipe_times_ms[8][2] = {};
  unsigned pipe_times_n = 0;
  uint64_t generation = 0;         // distinguishes contexts that reuse an address (key sets compare it)
  char err[512] = {0};
};

// Most items one call takes: the worklist entries of the ladder kernels carry a 2-bit tag above a 30-bit index (WL_TAG_LIMIT,
// engine_internal.h), so an index with bit 30 set must never reach them.
constexpr size_t S2K_MAX_BATCH = (size_t)1 << 30;

#include <atomic>
inline std::atomic<size_t>& s2k_internal_key_table_limit() {   // s2k_set_table_memory_budgets (engine.hip), read by keyed.hip
  static std::atomic<size_t> v{0};
  return v;
}
extern "C" size_t s2k_internal_keyset_budget();     // engine.hip: the keyset_free_bytes of s2k_set_table_memory_budgets (0: none)
gt_view s2k_internal_gt_load(const s2k_ctx* ctx);   // gtable.hip: the generator table a call that starts now uses (one load per call)
size_t s2k_internal_gt_pending_bytes(int device);   // gtable.hip: device memory the background table build is about to allocate
// a context's reference on its device's tables (fixed_bits == 0: the shared automatic tables - first table now, wide table in
// the background; else exactly that width), and the test hook behind s2k_debug_gt_swap_in_call: `bits` becomes the width of
// the device's automatic contexts now
hipError_t s2k_internal_gt_acquire(int device, int fixed_bits);
void s2k_internal_gt_release(int device);
hipError_t s2k_internal_gt_debug_publish(int device, int bits);

inline thread_local char g_err[512];

inline int fail(s2k_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (ctx) snprintf(ctx->err, sizeof ctx->err, "%s", buf);
  snprintf(g_err, sizeof g_err, "%s", buf);
  return code;
}
#define HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) return fail(ctx, S2K_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

// grow-only device buffer owned by the context
inline int ctx_reserve(s2k_ctx* ctx, void** p, size_t* have, size_t need) {
  if (need <= *have) return S2K_OK;
  if (*p) {
    HIP_TRY(ctx, hipFree(*p));
    *p = nullptr;
    *have = 0;
  }
  HIP_TRY(ctx, hipMalloc(p, need));
  *have = need;
  return S2K_OK;
}
static inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }
// lane stride of the [word][lane] planes: n rounded up to a wave, plus S2K_STRIDE_PAD lanes so
// that consecutive planes need not start at the same power-of-two offset
#ifndef S2K_STRIDE_PAD
#define S2K_STRIDE_PAD 0
#endif
static inline size_t lane_stride(size_t n) { return ((n + 63) & ~(size_t)63) + S2K_STRIDE_PAD; }


// Serialisation of the calls of one context across streams (see s2k_ctx::ev_done).
inline int ctx_enter(s2k_ctx* ctx, hipStream_t st) {
  ctx->gt_call = s2k_internal_gt_load(ctx);   // every launch of this call reads this view and no other
  if (ctx->have_last && ctx->last_stream != st) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_done, 0));
  return S2K_OK;
}
void s2k_internal_gt_kick(int device);      // gtable.hip: a call has been enqueued on the device (the background table build may start)
inline int ctx_leave(s2k_ctx* ctx, hipStream_t st) {
  s2k_internal_gt_kick(ctx->device);
  HIP_TRY(ctx, hipEventRecord(ctx->ev_done, st));
  ctx->last_stream = st;
  ctx->have_last = true;
  return S2K_OK;
}
// grid of the complete-formula worklist kernels: enough workgroups for the whole batch when
// every lane is undecided (adversarial input), at most 8 per CU (they loop over the list)
static inline unsigned fallback_blocks(const s2k_ctx* ctx, size_t n) {
  size_t want = (n + 255) / 256, cap = (size_t)(ctx->cu_count > 0 ? ctx->cu_count : 256) * 8;
  return (unsigned)(want < cap ? want : cap);
}

// second / third stream of the grouped flows and of the BIP-340 whole-batch check, with the events that fork and join them
inline int ctx_aux_streams(s2k_ctx* ctx) {
  if (ctx->ev_fork) return S2K_OK;
  if (!ctx->s_aux) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_aux, hipStreamNonBlocking));   // (a child context is given its parent's)
  // The third stream only where it is used (the two-part flow, off by default): the runtime multiplexes a process's
  // streams onto four hardware queues, and with the caller's stream, the copy stream and the compute stream a fifth one
  // made two of them share a queue - when those were the copy and a compute stream, the host-buffer path lost its
  // overlap (2^20 verifications from pinned memory: 9.3 instead of 7.3 ms, in some processes and not in others).
  if (ctx->kg_parts > 1 && !ctx->s_aux2) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_aux2, hipStreamNonBlocking));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_mid, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_part0, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_part1, hipEventDisableTiming));
  return S2K_OK;
}
// after a fork: whatever happened, the caller's stream waits for the second one again (an error return must not leave
// work of this call in flight on a stream the next call does not wait for)
inline void ctx_aux_join(s2k_ctx* ctx, hipStream_t st) {
  if (!ctx->s_aux) return;
  (void)hipEventRecord(ctx->ev_join, ctx->s_aux);
  (void)hipStreamWaitEvent(st, ctx->ev_join, 0);
}

// (the multiscalar core's host interface, its stage timing included: msm_internal.h)

// submit / wait plumbing (pipeline.hip), shared by the entry points that issue tickets (engine.hip, keyset.hip, digest.hip, ingest.hip)
int s2k_internal_pipe_slot(s2k_ctx* ctx, size_t n, uint8_t* valid, s2k_ctx::pipe_slot** out);   // free slot for the next ticket
int s2k_internal_pipe_retire(s2k_ctx* ctx, s2k_ctx::pipe_slot& sl);                             // wait + deliver verdicts
void s2k_internal_pipe_issue(s2k_ctx* ctx, s2k_ctx::pipe_slot* sl, uint64_t* ticket);
void s2k_internal_drain(s2k_ctx* ctx);                                                          // after an error: nothing left in flight
bool s2k_internal_host_pinned(const void* p, size_t bytes);
// small synchronous host calls without DMA transfers (pipeline.hip)
bool s2k_internal_small_call(const s2k_ctx* ctx, size_t n, uint32_t flags);
int s2k_internal_small_block(s2k_ctx* ctx, const size_t* sizes, int count, uint8_t** host, uint8_t** dev);

// Staging around a device form, for the host-pointer entry points that move their arrays whole (pipeline.hip).  A part is one
// array: `reserve` bytes of the context's staging buffer, of which `bytes` come from `src` before the device form runs (an
// input; nothing is copied for a null src or no bytes) or go to `dst` after it (a result).  `run` enqueues the device form on
// the staged pointers d[0 .. count) and the stream it is given, for the context it is given.
//   s2k_internal_staged_call    synchronous.  small: the page-locked block of s2k_internal_small_block, memcpy both ways, no
//                               DMA; else copies, phase guard of `phase_bytes` and device form on s_comp, then the wait
//   s2k_internal_staged_submit  the ticket form: a slot for n verdicts to `valid`, the copies in on the child's s_copy,
//                               chained by ev_copied[0] into its s_comp; the result part lands in the slot's landing buffer
// A device form that fails after copies were enqueued leaves the context drained (s2k_internal_drain) on every route.
struct stage_part {
  const void* src;
  void* dst;
  size_t bytes, reserve;
};
inline stage_part stage_in(const void* src, size_t bytes) { return {src, nullptr, bytes, bytes}; }
inline stage_part stage_in(const void* src, size_t bytes, size_t reserve) { return {src, nullptr, bytes, reserve}; }
inline stage_part stage_out(void* dst, size_t bytes) { return {nullptr, dst, bytes, bytes}; }
constexpr int STAGE_MAX_PARTS = 7;   // (s2k_ecdsa_recover_address_messages_batch: messages, offsets, r, s, ids, addresses, ok)
class stage_run {      // a reference to the caller's lambda int(s2k_ctx* c, uint8_t* const* d, hipStream_t st), good for the call it is passed to
  const void* f_;
  int (*call_)(const void*, s2k_ctx*, uint8_t* const*, hipStream_t);

 public:
  template <class F>
  stage_run(const F& f) : f_(&f), call_([](const void* p, s2k_ctx* c, uint8_t* const* d, hipStream_t st) { return (*static_cast<const F*>(p))(c, d, st); }) {}
  int operator()(s2k_ctx* c, uint8_t* const* d, hipStream_t st) const { return call_(f_, c, d, st); }
};
int s2k_internal_staged_call(s2k_ctx* ctx, const stage_part* parts, int count, size_t phase_bytes, bool small, const stage_run& run);
int s2k_internal_staged_submit(s2k_ctx* ctx, size_t n, uint8_t* valid, const stage_part* parts, int count, const stage_run& run,
                               s2k_ticket* ticket);
// the parts of a host form's messages: the blob (16 bytes of slack behind it, as the other message calls keep) and the offsets
inline stage_part part_msgs(const uint8_t* msgs, size_t total) { return stage_in(msgs, total, total + 16); }
inline stage_part part_offs(const uint64_t* offs, size_t n) { return stage_in(offs, offs ? (n + 1) * 8 : 0, offs ? (n + 1) * 8 : 8); }
constexpr size_t DG_SMALL_BYTES = (size_t)1 << 20;   // most message bytes a small call moves through the page-locked block
// digest.hip, for address.hip: what every messages form checks before anything is launched (host: the offsets are scanned,
// *total = the bytes to upload), and the digests of a call's messages into the context's buffer on `st`
int s2k_internal_msg_args(s2k_ctx* ctx, int alg, size_t n, const void* msgs, const uint64_t* msg_offsets, size_t msg_len, bool host, size_t* total);
int s2k_internal_digest_to_ctx(s2k_ctx* ctx, hipStream_t st, int alg, size_t n, const void* d_msgs, const void* d_offs, size_t msg_len,
                               const uint8_t** dig);

// Synchronous host-pointer entry points are transfer, kernels, answer in series.  Two verifiers (two contexts on two host
// threads) that take whole batches alternately could hide one's transfer behind the other's kernels, but left alone they fall
// into lock step - both copy, then both compute.  So the PHASES of such calls take turns per device: one call's transfer in,
// one call's kernels (and answer out) at a time.  s2k_phase_transfer locks the transfer phase of a call that moves at least
// PHASE_MIN_BYTES (smaller calls: no-op guards); `landed()` waits for the copies on the stream and hands over to the kernel
// phase.  A lone verifier meets no contention; what it pays is that its kernels are enqueued once its copies have landed
// instead of behind them on the stream (tens of microseconds).  Measured: DESIGN.md section 5.
struct s2k_phase_locks {
  std::mutex xfer, comp;
};
s2k_phase_locks& s2k_internal_phase(int device);          // engine.hip
constexpr size_t S2K_PHASE_MIN_BYTES = (size_t)4 << 20;
struct s2k_phase_guard {
  s2k_phase_locks& ph;
  bool on;
  std::unique_lock<std::mutex> x, c;
  s2k_phase_guard(int device, size_t bytes) : ph(s2k_internal_phase(device)), on(bytes >= S2K_PHASE_MIN_BYTES), x(ph.xfer, std::defer_lock), c(ph.comp, std::defer_lock) {
    if (on) x.lock();
  }
  // the copies are enqueued on `st`: wait for them, let the next call transfer, take the kernel phase
  hipError_t landed(hipStream_t st) {
    if (!on) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(st);
    x.unlock();
    c.lock();
    return e;
  }
};

// copy / compute streams and the events chaining them, for the host-buffer entry points
inline int ctx_streams(s2k_ctx* ctx) {
  if (!ctx->s_copy) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_copy, hipStreamNonBlocking));   // (a child context is given its parent's streams)
  if (!ctx->s_comp) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->s_comp, hipStreamNonBlocking));
  for (hipEvent_t& e : ctx->ev_copied)
    if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return S2K_OK;
}

inline int ctx_arrival_events(s2k_ctx* ctx) {
  for (hipEvent_t& e : ctx->ev_arrival)
    if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return S2K_OK;
}

// carve `count` buffers (256-byte aligned) out of the context's staging allocation, grown on demand:
// the host-buffer entry points stage their inputs and outputs here instead of allocating per call
inline int ctx_stage(s2k_ctx* ctx, const size_t* sizes, int count, uint8_t** ptrs) {
  size_t total = 0;
  for (int i = 0; i < count; ++i) total += (sizes[i] + 255) & ~(size_t)255;
  int rc = ctx_reserve(ctx, &ctx->io, &ctx->io_bytes, total + 256);
  if (rc) return rc;
  size_t off = 0;
  for (int i = 0; i < count; ++i) {
    ptrs[i] = (uint8_t*)ctx->io + off;
    off += (sizes[i] + 255) & ~(size_t)255;
  }
  return S2K_OK;
}

// ---- repeated-key path (keyed.hip; the ladder itself is k_verify_fast<MODE_ECDSA_KEYED>, verify_fast.h) ----
// A key that signs several signatures of a batch gets ONE table, built once: for each of the eight
// 16-bit chunks c of a 128-bit half scalar the odd multiples {1,3,..,15} * 2^(16c) Q, and 2^116 Q for
// the recoding's leading digit, all affine (one shared inversion per key) with their beta*x column.
// A signature's ladder is then 12 doublings instead of 128 around the same 66 additions.
// Two geometries.  CHUNKS = 8: what a verification call builds for itself (16-bit chunks, 12 doublings left per signature,
// 9 KiB per key).  CHUNKS = 32: key sets (s2k_keyset_*), built once, so their size is free: one chunk per 4-bit digit,
// {1,3,..,15} * 2^(4c) Q for c < 32 and the lead pair from L = 2^128 Q - a signature's ladder is 64 additions and NO
// doubling (36 KiB per key).
template <int CHUNKS>
struct kt_geom {
  static constexpr int DBL = 128 / CHUNKS;          // doublings from one chunk's base to the next (then 4 more to the lead point)
  static constexpr int LEAD_DBL = 4;
  static constexpr int LEAD = CHUNKS * 8;           // entries of L + phi(L) and (LEAD + 1) L - phi(L): the two starting points of a ladder
  static constexpr int ENTRIES = LEAD + 2;
  static constexpr int SCR = ENTRIES;               // first scratch entry; three field elements per entry (keyed.hip: kt_scratch)
  static constexpr int W_SLOT = CHUNKS + 1;         // scratch element that stays part of the table: W, the Z all entries of the key share
  static constexpr int PRE_SLOT = CHUNKS + 2;       // (32 chunks) prefix products of the nine / 33 Z, CHUNKS + 1 of them
  static constexpr int SCR_ELEMS = CHUNKS == 8 ? 18 : 2 * CHUNKS + 3;
  static constexpr int SLOTS = CHUNKS == 8 ? 72 : ((ENTRIES + (SCR_ELEMS + 2) / 3 + 7) / 8 * 8);   // entries of 128 bytes reserved per key
};
constexpr int KT_CHUNKS = 8;
constexpr int KT_LEAD = kt_geom<8>::LEAD;
constexpr int KT_ENTRIES = kt_geom<8>::ENTRIES;
constexpr int KT_SLOTS = kt_geom<8>::SLOTS;     // 72: 66 + 6 of build scratch
constexpr int KT_SCR = kt_geom<8>::SCR;
constexpr int KT_W_SLOT = kt_geom<8>::W_SLOT;   // 9
constexpr int KS_CHUNKS = 32;                   // key sets
constexpr int KS_SLOTS = kt_geom<32>::SLOTS;    // 288
// Key sets, JOINT tables: for every digit position c the sums E_a + s phi(E_b) of the chunk's odd multiples (a, b < 8, s = +-),
// so that the two half scalars' digits at a position cost ONE table addition: 32 additions per signature instead of 64.
// 128 entries per position, 80 bytes each (x and y of an affine point of the key's isomorphic curve: five quads
// [x 0-3][x 4-7][y 0-3][y 4-7][x8, y8, -, -]), 4096 entries = 320 KiB per key, built once from the 32-chunk table.
constexpr int KJ_ENTRY_QUADS = 5;
constexpr int KJ_PER_CHUNK = 128;
constexpr size_t KJ_KEY_QUADS = (size_t)KS_CHUNKS * KJ_PER_CHUNK * KJ_ENTRY_QUADS;   // 20480 quads = 320 KiB
// Wider joint tables (S2K_KEYSET_JOINT5 / S2K_KEYSET_JOINT6): the same idea on W-bit digits.  A half scalar k (odd, < 2^129) is
// k = 2^(W POS) + sum_i d_i 2^(W i), d_i = 2 w_i - (2^W - 1), w_i the W-bit windows of (k - 1) / 2, POS = ceil(128 / W) of them;
// per position the sums (2a + 1) B_i + s phi((2b + 1) B_i), a, b < 2^(W-1), s = +-, B_i = 2^(W i) Q: POS additions per signature
// instead of 32 (26 at W = 5, 22 at W = 6) for 2^(2W - 1) entries per position (0.81 MiB / 2.75 MiB per key).  The points are
// derived from the key's 32-chunk table by affine doublings and additions, so they live on the same isomorphic curve (same W
// factor at the end of the ladder).  The ladder's two starting points, 2^(W POS) Q +- phi(2^(W POS) Q), follow the positions.
template <int W>
struct kjw_geom {
  static constexpr int NE = 1 << (W - 1);                        // odd multiples per position
  static constexpr int POS = (128 + W - 1) / W;                  // digit positions
  static constexpr int PER_POS = NE * NE * 2;                    // joint entries per position
  static constexpr size_t LEAD = (size_t)POS * PER_POS;          // entries LEAD, LEAD + 1: the lead pair
  // entries of 64 bytes: x and y as eight 32-bit words each (canonical values; converted to limbs on load: 34 instructions
  // per lookup), so that a lookup is ONE aligned 64-byte fetch where an 80-byte entry of limbs straddles two or three
  static constexpr int EQ = 4;
  static constexpr size_t KEY_QUADS = (LEAD + 2) * EQ;
  static constexpr int LEAD_SHIFT = W * POS - 128;               // doublings from the chunk table's L = 2^128 Q to 2^(W POS) Q
};
static_assert(KT_SLOTS == 72 && KT_W_SLOT == 9 && kt_geom<32>::SLOTS == 288, "table geometry");
// The per-call tables of the ECDSA and BIP-340 flows, and the tables of a comb key set, as a signed Lim-Lee COMB (keyed.hip:
// k_key_chain<XONLY, 7> / k_key_finish_comb; the ladder is k_verify_fast<MODE_ECDSA_COMB> / <MODE_SCHNORR_COMB>, verify_fast.h).  An odd half scalar k < 2^129 is k = 2^L + sum_{i<L} b_i 2^i with
// b_i = 2 a_i - 1, a = (k - 1) / 2, for any L >= 128.  With L = TEETH * SPACING = 133 and i = 19 t + j the bits of column j
// select +-E[idx], E[idx] = B_6 + sum_{t<6} (2 idx_t - 1) B_t, B_t = 2^(19 t) Q (the sign is the top tooth's; a negative top
// tooth complements idx): 19 additions and 18 doublings per half, the doublings shared by the two halves - 38 additions and
// 18 doublings per signature from the same 64 entries + lead pair (L + phi(L), L - phi(L), L = 2^115 Q) the window tables hold.
// The default ladder, k_verify_comb (comb_ladder.hip), takes the lead as a digit instead - a' = a | 2^(L-1), the top tooth's
// bit 18: sum_{i<L} (2 a'_i - 1) 2^i = k with no 2^L in front - and reads the 64 entries only; the lead pair stays in the table
// for k_verify_fast<MODE_.._COMB> (S2K_COMB_LEAD=1).
struct kc_geom {
  static constexpr int TEETH = 7, SPACING = 19, LEN = TEETH * SPACING;
  static constexpr int LEAD_LOG2 = LEN - SPACING + 1;   // 115: the ladder's 18 doublings make the lead 2^133 Q
  static constexpr int LEAD = 64, ENTRIES = 66;
  // what k_key_chain reads of a geometry: SPACING doublings from one base to the next, one more to the lead point; the
  // Jacobian bases B_t parked in the entries BASE_STEP * t until kc_sets (keyed.hip) has read them all
  static constexpr int DBL = SPACING, LEAD_DBL = 1, BASE_STEP = 8;
  // build scratch behind the entries: what k_key_finish_comb reads of a key - A_i = B_6 +- B_5 +- B_4 in ASET + i,
  // C_j = B_3 +- B_2 +- B_1 +- B_0 in CSET + j (x, y over one common Z) and that Z in element ZAC of entry WENT, whose
  // element W stays part of the table (the Z all entries of the key share).  Its lanes overwrite the entries while others
  // still read these twelve points, hence not inside the 64: 80 slots of 128 bytes per key against the window tables' 72
  // (66 + 6 of scratch), 10 KiB instead of 9.
  static constexpr int ASET = ENTRIES, CSET = ASET + 4, WENT = CSET + 8, W = 0, ZAC = 1;
  static constexpr int SLOTS = 80;
};
template <>
struct kt_geom<kc_geom::TEETH> : kc_geom {};
constexpr int KC_TEETH = kc_geom::TEETH;        // key_groups::chunks of a call on comb tables
constexpr int KC_SLOTS = kc_geom::SLOTS;
static_assert(kc_geom::LEN == 133 && kc_geom::LEAD_LOG2 == 115 && (kc_geom::TEETH - 1) * kc_geom::SPACING + 1 == kc_geom::LEAD_LOG2 &&
              kc_geom::WENT < kc_geom::SLOTS && kc_geom::BASE_STEP * (kc_geom::TEETH - 1) < kc_geom::LEAD && KC_SLOTS >= KT_SLOTS, "comb geometry");
static_assert(kjw_geom<5>::POS == 26 && kjw_geom<5>::LEAD_SHIFT == 2 && kjw_geom<6>::POS == 22 && kjw_geom<6>::LEAD_SHIFT == 4, "joint geometry");
enum { KG_NKEYED = 0, KG_NTAB = 1, KG_NLEFT = 2, KG_SPLIT_T = 3, KG_SPLIT_LANE = 4, KG_ALLOC64 = 6 /* and 7 */, KG_COUNTERS = 16 };
constexpr uint32_t KG_NONE = 0xffffffffu;
constexpr size_t KG_MIN_BATCH = 256;            // smaller batches skip the grouping
// S2K_KEYS_ADAPTIVE (s2k_ctx above): batches it learns from and applies to, misses before it stops looking, batches it then skips
constexpr size_t KG_ADAPT_MIN_BATCH = (size_t)1 << 16;
constexpr uint32_t KG_ADAPT_MISSES = 2, KG_ADAPT_SKIP = 15, KG_ADAPT_SLOTS = 8;
// Signatures per key from which a table pays, measured (MI355X, 2^20 signatures, ms with tables / without):
// 4 per key 7.94 / 8.02, 5 per key 8.08 / 8.01 (the table kernels do not scale linearly and the clock sags),
// 6 per key 6.65 / 7.93, 8 per key 6.02 / 7.96, 16 per key 5.1 / 8.0
constexpr uint32_t KG_MIN_GROUP = 4;   // measured break-even: 4 per key 7.78 against 8.14 ms without tables, 3 per key no gain
struct key_groups {        // device pointers of one call
  uint32_t* counters;      // [KG_NKEYED] signatures on the keyed path, [KG_NTAB] tables, [KG_NLEFT] the rest
  uint32_t* perm;          // keyed lane -> signature
  uint32_t* ptab;          // keyed lane -> table
  uint32_t* left;          // dense lane of the general kernel -> signature
  const uint4* ktab;       // tables, KT_SLOTS * 8 quads each
  const uint4* jtab;       // key sets with joint tables: KJ_KEY_QUADS quads per key (else null)
  const uint8_t* tinfo;    // per table: 1 if the key is a valid public key
  const uint32_t* trep;    // per table: a signature that carries the key
  const uint32_t* gp;      // per signature: u1*G (Jacobian, three fin-format elements; k_generator_part)
  uint32_t max_tables;
  int chunks;              // table geometry: 8 (built per call) or 32 (key sets); 0 means 8; KC_TEETH (7): the comb tables of a call or of a comb key set
  int key_bytes;           // 64: X || Y (ECDSA), 32: x-only (BIP-340)
  // two-part flow: part 0 = tables [0, counters[KG_SPLIT_T]) and lanes [0, counters[KG_SPLIT_LANE]), part 1 the
  // rest; nparts == 1: everything (kernels take these from the copy of the struct they are launched with)
  uint32_t part, nparts;
};
// groups the batch's signatures by public key, then builds the tables (enqueue only, no host sync); the tables' geometry
// (out->chunks) is the comb's when ctx->kt_comb_call (and S2K_KEY_TABLES_SPLIT is not set), else the 16-bit chunks'
int s2k_internal_key_group(s2k_ctx* ctx, size_t n, const uint8_t* d_pub, int key_bytes, hipStream_t st, key_groups* out);
int s2k_internal_key_reserve(s2k_ctx* ctx, size_t n, int key_bytes);   // grow the grouping arrays / table buffer (before any fork)
size_t s2k_internal_key_bytes(const s2k_ctx* ctx, size_t n);            // what those hold for a batch of n
int s2k_internal_key_chains(s2k_ctx* ctx, const uint8_t* d_pub, hipStream_t st, const key_groups* g);
// (ev_mid, if any, is recorded on st where the rest of the generator part may start beside the tables: in front of
// k_key_finish; with the three kernels of S2K_KEY_TABLES_SPLIT and for a key set between k_key_odd and k_key_cofactors)
int s2k_internal_key_tables(s2k_ctx* ctx, hipStream_t st, const key_groups* g, uint32_t part, uint32_t nparts,
                            hipEvent_t ev_mid);

// grouping of x-only keys for the BIP-340 whole-batch check (rlc.hip): every key a group, long groups cut
// into virtual groups of KG_VGROUP signatures
constexpr uint32_t KG_VGROUP = 1024;
struct key_groups32 {
  const uint32_t *rep, *cnt, *base, *tix;   // per hash slot: first signature, size, first sorted position, first virtual group
  const uint32_t* perm;                     // sorted position -> signature
  const uint32_t* left;                     // signatures whose key found no slot (each is its own group)
  const uint32_t* vslot;                    // virtual group -> slot
  uint32_t ngroups, nleft;                  // (host values)
};
int s2k_internal_key_group32(s2k_ctx* ctx, size_t n, const uint8_t* d_pk32, hipStream_t st, key_groups32* out);
// the same grouping for keys of key_bytes = 32 (x-only) or 64 (X || Y, the recoverable-ECDSA whole-batch check): every one
// of the key's bytes is compared
int s2k_internal_key_group_all(s2k_ctx* ctx, size_t n, const uint8_t* d_keys, int key_bytes, hipStream_t st, key_groups32* out);
int s2k_internal_key_reserve32(s2k_ctx* ctx, size_t n);
// key sets (s2k_keyset_*): buffer layout, table build, scratch reservation, sort of a batch by key index
// (chunks: the geometry of the set's tables, KS_CHUNKS - also what the joint layouts are built from - or KC_TEETH, a comb set)
// (cap: the capacity the set's buffers are laid out for, s2k_keyset_capacity; first, count: a range of its keys; nkeys: its live keys)
size_t s2k_internal_keyset_bytes(size_t cap, size_t off[5], int chunks = KS_CHUNKS);
// the sections of a set's buffer, laid out for its capacity (the only reader of those five offsets besides the byte total)
struct keyset_view {
  uint8_t* keys;         // X || Y, 64 bytes per key
  uint4* tables;         // the 32-chunk or comb tables: KS_SLOTS or KC_SLOTS entries of 128 bytes per key
  uint8_t* valid;        // one byte per key: it is a public key (rows past the live keys: 0)
  uint32_t* rep;         // the identity 0 .. cap - 1 (what key_groups::trep is for a set: table t is the key of "signature" t)
  uint32_t* counters;    // KG_COUNTERS words: scratch of the table builds
};
inline keyset_view s2k_internal_keyset_view(const uint8_t* base, size_t cap, int chunks = KS_CHUNKS) {
  size_t off[5];
  (void)s2k_internal_keyset_bytes(cap, off, chunks);
  uint8_t* b = const_cast<uint8_t*>(base);      // (a caller that holds the set const only reads through the view)
  return {b + off[0], (uint4*)(b + off[1]), b + off[2], (uint32_t*)(b + off[3]), (uint32_t*)(b + off[4])};
}
int s2k_internal_keyset_build(s2k_ctx* ctx, uint8_t* base, size_t cap, size_t first, size_t count, hipStream_t st, int chunks = KS_CHUNKS);
int s2k_internal_keyset_identity(s2k_ctx* ctx, uint8_t* base, size_t cap, hipStream_t st, int chunks = KS_CHUNKS);
int s2k_internal_keyset_build_joint(s2k_ctx* ctx, const uint8_t* base, size_t cap, size_t first, size_t count, uint4* joint, hipStream_t st);   // from the 32-chunk tables
size_t s2k_internal_keyset_joint_bytes(size_t n, int w);                  // joint tables of n keys at digit width w (4, 5, 6)
size_t s2k_internal_keyset_joint_scratch_bytes(size_t n, int w);          // build scratch of the wide layouts (0 at w = 4)
int s2k_internal_keyset_build_joint_wide(s2k_ctx* ctx, const uint8_t* base, size_t cap, size_t first, size_t count, int w, uint4* joint, uint4* scratch, hipStream_t st);
int s2k_internal_keyset_reserve(s2k_ctx* ctx, size_t nkeys, size_t n);
int s2k_internal_keyset_sort(s2k_ctx* ctx, const uint8_t* set_base, size_t cap, size_t nkeys, size_t n, const uint32_t* d_kidx, hipStream_t st,
                             key_groups* out, int chunks = KS_CHUNKS);
// replacing rows of a set (keyset_replace.hip; s2k_keyset_replace, keyset.hip): the host plan of a call (s2k_debug_keyset_replace_plan),
// the keys of a piece for a layout, and the rows 0 .. count - 1 of a staging set moved to the rows d_slots[] of the set
int s2k_internal_keyset_replace_plan(size_t n_live, size_t m, const uint32_t* slots, size_t piece_keys, uint32_t* order, uint64_t* n_pieces);
size_t s2k_internal_keyset_replace_piece(int chunks, int jw);
int s2k_internal_keyset_scatter_rows(const uint8_t* stage, size_t stage_cap, const uint4* stage_joint, uint8_t* base, size_t cap, uint4* joint,
                                     int jw, int chunks, const uint32_t* d_slots, size_t count);

// the index of a key set, key bytes -> key index (keyset_index.hip; the table and its probe loops: keyset_index.h).  Enqueue
// only.  build: inserts the keys first .. first + count - 1; `slots` (2^log2_slots words of 64 bits) all ones and `info`
// (S2K_KSI_INFO_WORDS words) zero before the first range, and left as the earlier ranges left them before a later one;
// lookup: d_out[i] = the index of the set's key equal to the key_bytes (64: X || Y, 32: X) bytes at d_keys + i * stride, else
// 0xFFFFFFFF.  key_bytes S2K_KSI_X_VALID: 32 bytes of X looked up among the set's VALID keys only (ksi_lookup32v: the fused
// BIP-340 call's lookup; s2k_keyset_lookup* never passes it)
enum { S2K_KSI_OCCUPIED = 0, S2K_KSI_LONGEST = 1, S2K_KSI_FAILED = 2, S2K_KSI_INFO_WORDS = 4 };
constexpr int S2K_KSI_X_VALID = -32;
int s2k_internal_ksi_build(s2k_ctx* ctx, hipStream_t st, const uint8_t* set_keys, size_t first, size_t count, uint64_t* slots, uint32_t log2_slots,
                           uint64_t seed, uint32_t* info);
int s2k_internal_ksi_lookup(s2k_ctx* ctx, hipStream_t st, const uint8_t* set_keys, const uint64_t* slots, uint32_t log2_slots, uint64_t seed,
                            const uint8_t* key_valid, size_t n, const uint8_t* d_keys, int key_bytes, size_t stride, uint32_t* d_out);

// ECDSA by key bytes over a key set, for the encoded entry points (ingest.hip; engine.hip owns the set).
//   s2k_internal_bykey_view      what s2k_ecdsa_verify_batch_keyset_bykey asks of its set and flags (own context, an index, no
//                                S2K_ECDSA_FORCE_COMPLETE), then what a kernel needs to probe the set's index
//   s2k_internal_bykey_delegates the plain call would take its wave-per-signature or four-lanes-per-signature ladder for this
//                                n: the set is not used
//   s2k_internal_bykey_device    s2k_ecdsa_verify_batch_keyset_bykey_device past its checks, never delegating.  d_found:
//                                null, or the key indices of the n signatures already resolved (0xFFFFFFFF: not in the set;
//                                the lookup launch is skipped) - ctx->ks_found, reserved and filled by the caller on `st`
struct s2k_bykey_view {
  keyset_view set;            // the set's buffer: the probe reads `keys` and `valid`
  uint64_t* slots;            // the index
  uint32_t log2_slots;
  uint64_t seed;
};
int s2k_internal_bykey_view(s2k_ctx* ctx, const s2k_keyset* ks, uint32_t flags, s2k_bykey_view* out);
bool s2k_internal_bykey_delegates(const s2k_ctx* ctx, size_t n, uint32_t flags);
int s2k_internal_bykey_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_pub_xy, const void* d_dig, const void* d_r,
                              const void* d_s, uint32_t flags, void* d_valid, hipStream_t st, const uint32_t* d_found);

// ---- engine.hip, lane_kernels.hip, fallback.hip, worklist.hip and small_call.hip, for each other and for the key-set flows (keyset.hip): ladder modes, the lane workspace,
// stage-timing marks and launchers ----
enum { MODE_ECDSA = 0, MODE_SCHNORR = 1, MODE_RECOVER = 2, MODE_POINT = 3, MODE_ECDSA_KEYED = 4, MODE_ECDSA_LEFT = 5,
       MODE_SCHNORR_KEYED = 6, MODE_SCHNORR_LEFT = 7, MODE_ECDSA_KEYSET = 8, MODE_ECDSA_KEYSET_JOINT = 9,
       MODE_ECDSA_KEYSET_JOINT5 = 10, MODE_ECDSA_KEYSET_JOINT6 = 11,
       // BIP-340 over a key set's tables, same four layouts: the ECDSA mode + 4
       MODE_SCHNORR_KEYSET = 12, MODE_SCHNORR_KEYSET_JOINT = 13, MODE_SCHNORR_KEYSET_JOINT5 = 14, MODE_SCHNORR_KEYSET_JOINT6 = 15,
       // MODE_ECDSA_KEYED over the key's COMB table (kc_geom): 38 additions and 18 doublings.  New modes go at the end:
       // tools/isa_count.py finds the kernels by this number
       MODE_ECDSA_COMB = 16,
       // MODE_SCHNORR_KEYED over the comb table (the lifted x-only keys of a call, or the X || Y keys of a comb key set)
       MODE_SCHNORR_COMB = 17 };
constexpr uint32_t KVF_FORCE_WORKLIST = 0x80000000u;   // top bit of k_verify_fast's first argument (batches are below 2^31)
// what the ladder kernels of verify_fast.h and comb_ladder.hip share:
// the flag word of a signature's prepared scalars (k_scalar_prep, plane 16)
enum { PF_OK = 1, PF_NEG1 = 2, PF_NEG2 = 4, PF_K1_B128 = 8, PF_K2_B128 = 16 };   // bit 128 of the odd half-scalars
// A worklist entry of the ECDSA flows is the signature's index, plus (batches below 2^30) a tag in the top bits:
// WL_DOUBLE_GEN = the fast ladder found u2 Q == u1 G, both finite, in its final addition: R = 2 u1 G;
// WL_DOUBLE_LAST = the plain ladder (generator part inside the kernel) found its sum equal to the last generator-table
// entry it was about to add: R = 2 T_last[top digit of u1].
constexpr uint32_t WL_TAG_LIMIT = 1u << 30, WL_INDEX_MASK = WL_TAG_LIMIT - 1u, WL_DOUBLE_GEN = 1u << 30, WL_DOUBLE_LAST = 2u << 30;
// The comb ladders: 145 VGPRs and three waves since a column adds its two entries to each other first; 4 here spills
// (128 VGPRs, 23 spilled, 64 B scratch) and was timed no faster than the two-addition column it replaced.
#ifndef S2K_COMB_WAVES
#define S2K_COMB_WAVES 3
#endif
// The bounds of the other ladders of k_verify_fast (measured: verify_fast.h) and the signatures that share an inversion in
// k_scalar_prep (measured: lane_kernels.hip).  Here because s2k_build_config (engine.hip) names them too.
#ifndef S2K_FAST_WAVES
#define S2K_FAST_WAVES 3
#endif
#ifndef S2K_JOINT_WAVES
#define S2K_JOINT_WAVES 3
#endif
#ifndef S2K_PREP_M
#define S2K_PREP_M 6
#endif
constexpr int PREP_WORDS = 17;                         // planes of a signature's prepared scalars (k_scalar_prep: u1, |k1|, |k2|, flags)
// Which kernel runs the comb ladders when S2K_COMB_LEAD is not set: 0 = k_verify_comb (comb_ladder.hip: no lead point, the
// first round is one pair sum), 1 = k_verify_fast<MODE_.._COMB> (verify_fast.h).  s2k_build_config() names it.
#ifndef S2K_COMB_LEAD_DEFAULT
#define S2K_COMB_LEAD_DEFAULT 0
#endif
constexpr uint8_t VERDICT_PENDING = 2;   // a ladder kernel -> k_affine_finish
constexpr int FIN_M = 16;                              // lanes per thread of k_affine_finish: its T argument is ceil(n / FIN_M)
// The planes of ctx->ws for a batch of n (layout: WS_* in engine.hip; lane_ws_of), after s2k_internal_ensure_ws(ctx, n).
struct lane_ws {
  uint32_t *qt, *fin, *prep, *gp, *pref, *smont, *wl_count, *wl;
  size_t stride;
};
extern "C" int s2k_internal_ensure_ws(s2k_ctx* ctx, size_t n);
// ct_cpu.cpp: out = a - b on 65-byte records (host; public data)
extern "C" __attribute__((visibility("hidden"))) int s2k_internal_point_sub65(const uint8_t* a, const uint8_t* b, uint8_t* out);
lane_ws lane_ws_of(const s2k_ctx* ctx, size_t n);
void prof_mark(s2k_ctx* ctx, hipStream_t st, int slot);       // s2k_ctx_profile: event `slot` of the call's six, on st
uint32_t prep_lanes(size_t n);                                // lanes of k_scalar_prep for n signatures
void launch_scalar_prep(hipStream_t st, const lane_ws& w, size_t first, size_t count, uint32_t lanes, const uint8_t* dig, const uint8_t* r,
                        const uint8_t* s, const uint8_t* recid, uint32_t flags);
void launch_generator_part(const s2k_ctx* ctx, hipStream_t st, const lane_ws& w, uint32_t first, uint32_t end);
void launch_ladder(const s2k_ctx* ctx, hipStream_t st, int mode, size_t n, uint32_t kvf, const uint8_t* pub, const uint8_t* rsig, const lane_ws& w,
                   uint8_t* out, uint8_t* out_pts, uint64_t* clk, const key_groups& kg);
// verify_fast.h: the ladder kernel, one instantiation per MODE_*, each in one of the ladder_*.hip units; launched by
// launch_ladder alone
template <int MODE>
__global__ void k_verify_fast(uint32_t n_and_flags, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ rsig,
                              const uint32_t* __restrict__ prep, uint32_t* __restrict__ qt, uint32_t* __restrict__ fin, gt_view gt,
                              uint8_t* __restrict__ out, uint32_t* __restrict__ wl_count, uint32_t* __restrict__ wl, size_t stride,
                              uint8_t* __restrict__ out_pts, uint64_t* __restrict__ clk, key_groups kg);
// comb_ladder.hip: the comb ladders without the lead point (the arguments of k_verify_fast); instantiated there for
// false (ECDSA) and true (BIP-340), launched by launch_ladder alone
template <bool SCHNORR>
__global__ void k_verify_comb(uint32_t n_and_flags, const uint8_t* __restrict__ pub, const uint8_t* __restrict__ rsig,
                              const uint32_t* __restrict__ prep, uint32_t* __restrict__ qt, uint32_t* __restrict__ fin, gt_view gt,
                              uint8_t* __restrict__ out, uint32_t* __restrict__ wl_count, uint32_t* __restrict__ wl, size_t stride,
                              uint8_t* __restrict__ out_pts, uint64_t* __restrict__ clk, key_groups kg);
void launch_affine_finish(hipStream_t st, int mode, size_t n, uint32_t T, const uint8_t* rsig, const lane_ws& w, uint8_t* out, uint8_t* out_pts);
void launch_verify_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                            const uint8_t* s, uint32_t flags, uint8_t* out);
void launch_verify_fallback_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* keys, const uint32_t* kidx,
                                   const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out);
void launch_schnorr_prep(hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs, const uint64_t* offs,
                         uint32_t msg_len);
void launch_schnorr_worklist(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig,
                             const uint8_t* msgs, const uint64_t* offs, uint32_t msg_len, uint8_t* out);
void launch_hot_prep(hipStream_t st, size_t n, const lane_ws& w, const uint8_t* u1, const uint8_t* u2, const uint8_t* pts65, uint8_t* pub64,
                     uint32_t* status);
// fallback.hip (with the three launch_*_fallback* / launch_schnorr_worklist above): the kernels that take every item through the
// complete formulas, and the recovery and point worklists
void launch_ecdsa_verify(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pub, const uint8_t* dig,
                         const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out);
void launch_schnorr_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* pk, const uint8_t* sig,
                             const uint8_t* msgs, const uint64_t* offs, uint32_t msg_len, uint8_t* out);
void launch_recover_fallback(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* dig, const uint8_t* r,
                             const uint8_t* s, const uint8_t* recid, uint8_t* ok, uint8_t* pub65);
void launch_recover_worklist(const s2k_ctx* ctx, hipStream_t st, size_t n, const lane_ws& w, const uint8_t* dig, const uint8_t* r,
                             const uint8_t* s, const uint8_t* recid, uint8_t* ok, uint8_t* pub65);
void launch_point_fallback(const s2k_ctx* ctx, hipStream_t st, bool all, size_t n, const lane_ws& w, const uint8_t* u1, const uint8_t* u2,
                           const uint8_t* pts65, uint8_t* out65, uint32_t* status);
// small_call.hip: the wave-per-signature kernels (launch_schnorr_row: prep == nullptr is k_schnorr_row<true>, whose fifth wave
// prepares; else the planes of launch_schnorr_prep) and the four-lanes-per-signature kernels, behind the preparation kernels
void launch_verify_row(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                       uint32_t flags, uint8_t* out);
void launch_schnorr_row(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* sig, const uint8_t* msgs,
                        const uint64_t* offs, uint32_t msg_len, const uint32_t* prep, size_t stride, uint8_t* out);
void launch_recover_row(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                        const uint8_t* recid, uint8_t* ok, uint8_t* pub65);
void launch_verify_quad(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pub, const uint8_t* r, const lane_ws& w, uint8_t* out);
void launch_schnorr_quad(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* pk, const uint8_t* sig, const lane_ws& w, uint8_t* out);
void launch_recover_quad(const s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* r, const lane_ws& w, uint8_t* out);
void launch_verify_row_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint4* ktab,
                              const uint8_t* tinfo, const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out);
void launch_schnorr_row_keyset(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint8_t* set_keys,
                               const uint4* ktab, const uint8_t* tinfo, const uint8_t* sig, const uint8_t* msgs, const uint64_t* offs,
                               uint32_t msg_len, uint8_t* out);
void launch_verify_row_comb(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint4* ktab,
                            const uint8_t* tinfo, const uint8_t* dig, const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* out);
void launch_schnorr_row_comb(const s2k_ctx* ctx, hipStream_t st, size_t n, size_t nkeys, const uint32_t* kidx, const uint8_t* set_keys,
                             const uint4* ktab, const uint8_t* tinfo, const uint8_t* sig, const uint8_t* msgs, const uint64_t* offs,
                             uint32_t msg_len, uint8_t* out);

struct dev_buf {
  void* p = nullptr;
  ~dev_buf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
  hipError_t upload(const void* src, size_t bytes) {
    hipError_t e = alloc(bytes);
    if (e != hipSuccess || !bytes) return e;
    return hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
  }
};

