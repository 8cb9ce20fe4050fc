// engine.hip — host code only: the context, the settings, the lane workspace, and the ECDSA, BIP-340, recovery and point call
// flows of include/secp256k1_voi_amd.h.  No kernel and no launch is in this file (tests/test_ladder_units_cpu.py).  Elsewhere:
//   verify_fast.h        the ladder kernel k_verify_fast<MODE>, one lane per signature
//   ladder_ecdsa.hip, ladder_schnorr.hip, fallback.hip   its instantiations, every MODE_* in one of them
//   lane_kernels.hip     k_scalar_prep, k_schnorr_prep, k_hot_prep, k_generator_part, k_affine_finish and their launchers;
//                        launch_ladder
//   fallback.hip         the complete-formula and worklist kernels and their launchers
//   comb_ladder.hip      the comb ladders without the lead point
//   small_call.hip       the kernels of calls too small for a lane per signature
//   pipeline.hip         host staging, tickets and page-locked memory
//   gtable.hip           the generator tables
//   keyset.hip           key sets and the entry points over them
//
// One lane per signature / per point; every lane of a wave runs the same instruction
// stream (complete formulas, fixed windows), so there is no divergence on secret- or
// data-dependent branches and no idle lanes.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include <sys/random.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "engine_internal.h"
#include "keyset_index.h"
#include "fe.h"
#include "fe29_inv.h"
#include "jacobian29.h"
#include "xyzz29.h"
#include "lane_tables.h"
#include "pt29.h"
#include "complete_path.h"
#include "point.h"
#include "sc.h"
#include "sc26.h"
#include "sig_prep.h"

using namespace s2k;

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
// per-stage timing (s2k_ctx_profile): six events per call, around scalar preparation | grouping and
// per-key tables | ladder (keyed, or the general one when grouping is off) | general ladder over the
// ungrouped rest | complete-formula worklist
constexpr int PROF_EV = 6;
__attribute__((visibility("hidden"))) void prof_mark(s2k_ctx* ctx, hipStream_t st, int slot) {
  if (!ctx->prof_on || ctx->prof_used + PROF_EV > ctx->prof_cap) return;
  (void)hipEventRecord(ctx->prof_ev[ctx->prof_used + slot], st);
  if (slot == PROF_EV - 1) ctx->prof_used += PROF_EV;
}

// Front end of the grouped flows (ECDSA and BIP-340 verification): everything up to the ladders.
// Caller's stream: grouping by key (k_key_insert / k_key_alloc / k_key_place), then the per-key tables.
// Second stream: the scalar preparation (`launch_prep`), then the generator part u1*G in two pieces.  These
// have nothing to do with the keys and the grouping / table kernels are short of work for the multipliers
// on their own (the doubling chain of the tables is one lane per KEY, the scaling pass is memory bound).
// The first piece of the generator part runs beside the chain, the second beside k_key_finish (its event sits in
// front of that kernel; between k_key_odd and k_key_cofactors where the three older kernels build the tables).  The
// share of the first piece (S2K_GP_FIRST_PERCENT, 60) is flat between 30 and 100 and costs 0.3 ms at 0
// (profiles/r07_key_finish_ab.txt).  Returns with the caller's stream waiting for the second.
// Stage times (s2k_ctx_profile_read_stages): [0] grouping, [1] tables and whatever is left of the second
// stream's work.
// S2K_KEYS_ADAPTIVE (engine_internal.h: kga_*): takes in the notes that have arrived, decides whether this call looks for
// repeated keys, and if it does, where its k_key_counts leaves its note.  No device call that waits.
static bool kg_adaptive_decide(s2k_ctx* ctx) {
  s2k_ctx* own = ctx->parent ? ctx->parent : ctx;
  if (!own->kga_note) {
    void* p = nullptr;
    if (hipHostMalloc(&p, KG_ADAPT_SLOTS * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return true;                                     // no note, no learning: S2K_KEYS_AUTO
    }
    memset(p, 0, KG_ADAPT_SLOTS * sizeof(unsigned long long));
    own->kga_note = (unsigned long long*)p;
  }
  for (;;) {                                           // notes in the order of their numbers; a slot overwritten by a later call: that one
    unsigned long long next = 0;
    for (uint32_t i = 0; i < KG_ADAPT_SLOTS; ++i) {
      const unsigned long long v = __atomic_load_n(&own->kga_note[i], __ATOMIC_ACQUIRE);
      const uint32_t sq = (uint32_t)(v >> 32);
      if (v && (int32_t)(sq - own->kga_seen) > 0 && (!next || (int32_t)(sq - (uint32_t)(next >> 32)) < 0)) next = v;
    }
    if (!next) break;
    own->kga_seen = (uint32_t)(next >> 32);
    ++own->kga_observed;
    if ((uint32_t)next == 0) {
      ++own->kga_miss_streak;
    } else {
      own->kga_miss_streak = 0;
      own->kga_skip_left = 0;
      own->kga_skipping = false;
    }
  }
  if (own->kga_miss_streak >= KG_ADAPT_MISSES) {
    if (!own->kga_skipping) {
      own->kga_skipping = true;
      own->kga_skip_left = KG_ADAPT_SKIP;
    }
    if (own->kga_skip_left) {
      --own->kga_skip_left;
      ++own->kga_skipped;
      return false;
    }
    own->kga_skip_left = KG_ADAPT_SKIP;                // this call looks again; the next ones do not, unless it finds something
    ++own->kga_probes;
  } else {
    own->kga_skipping = false;
  }
  if (++own->kga_seq == 0) own->kga_seq = 1;           // (0 marks an empty slot)
  ctx->kg_note_seq = own->kga_seq;
  ctx->kg_note_dst = own->kga_note + own->kga_seq % KG_ADAPT_SLOTS;
  return true;
}

template <class PrepFn>
static int grouped_front_forked(s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* d_keys, int key_bytes, const lane_ws& w,
                                PrepFn launch_prep, key_groups* kg, bool gp_in_prep) {
  // One stream (a child context of submit / wait): the grouping and the tables first - they need the keys only, which
  // arrive first -, then the preparation and the generator part; other tickets' kernels fill the machine meanwhile.
  const bool one_stream = ctx->s_aux == st;
  // gp_in_prep: the caller's launch_prep has enqueued the generator part as well (piecewise, as its inputs arrive)
  const uint32_t n_first = (gp_in_prep || one_stream) ? (gp_in_prep ? (uint32_t)n : 0u)
                                                      : (uint32_t)((n * (size_t)ctx->gp_first_percent / 100) & ~(size_t)255);
  if (!one_stream) {
    launch_prep(ctx->s_aux);
    HIP_TRY(ctx, hipGetLastError());
    if (n_first && !gp_in_prep) {
      launch_generator_part(ctx, ctx->s_aux, w, 0u, n_first);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  int rc = s2k_internal_key_group(ctx, n, d_keys, key_bytes, st, kg);
  if (rc) return rc;
  kg->gp = w.gp;
  kg->part = 0;
  kg->nparts = ctx->kg_parts;
  prof_mark(ctx, st, 1);
  rc = s2k_internal_key_chains(ctx, d_keys, st, kg);
  if (rc) return rc;
  // Two-part flow (S2K_KEYED_PARTS=2, off by default): the tables of the first half of the keys here; those
  // of the second half on a third stream, started when these are done, i.e. beside the first half's ladder.
  // Measured: the tables' share of the step shrinks by 0.3 ms and the ladders grow by 0.36 (2^16 keys: 5.27-5.30
  // against 5.22 ms; 2^17 keys: 6.33 against 6.12-6.21) - the table kernels' traffic costs the ladder more
  // than their idle multipliers give it.
  rc = s2k_internal_key_tables(ctx, st, kg, 0, kg->nparts, ctx->ev_mid);
  if (rc) return rc;
  if (kg->nparts > 1) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_part0, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux2, ctx->ev_part0, 0));
    rc = s2k_internal_key_tables(ctx, ctx->s_aux2, kg, 1, kg->nparts, nullptr);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_part1, ctx->s_aux2));
  }
  if (one_stream) {
    launch_prep(st);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux, ctx->ev_mid, 0));
  }
  if (n_first < n) {
    launch_generator_part(ctx, ctx->s_aux, w, n_first, (uint32_t)n);
    HIP_TRY(ctx, hipGetLastError());
  }
  return S2K_OK;
}
template <class PrepFn>
static int grouped_front(s2k_ctx* ctx, hipStream_t st, size_t n, const uint8_t* d_keys, int key_bytes, const lane_ws& w,
                         PrepFn launch_prep, key_groups* kg, bool gp_in_prep = false) {
  int rc = ctx_aux_streams(ctx);
  if (rc) return rc;
  // the buffers the grouping needs are reserved BEFORE the fork: growing one is a device-wide synchronisation
  // (hipFree), which must not meet work of this call in flight on the second stream
  rc = s2k_internal_key_reserve(ctx, n, key_bytes);
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux, ctx->ev_fork, 0));
  rc = grouped_front_forked(ctx, st, n, d_keys, key_bytes, w, launch_prep, kg, gp_in_prep);
  // error or not, the caller's stream waits for the second one again, and the context's next call for this one: an
  // error return leaves nothing of this call in flight behind the context's back
  ctx_aux_join(ctx, st);
  if (kg->nparts > 1 && rc == S2K_OK) { /* (ev_part1 is waited for by the caller, before the second ladder) */ }
  if (rc) {
    if (ctx->s_aux2) {
      (void)hipEventRecord(ctx->ev_part1, ctx->s_aux2);
      (void)hipStreamWaitEvent(st, ctx->ev_part1, 0);
    }
    (void)ctx_leave(ctx, st);
  }
  return rc;
}

s2k_phase_locks& s2k_internal_phase(int device) {
  static s2k_phase_locks locks[64];
  return locks[device & 63];
}

extern "C" {

const char* s2k_version(void) { return "secp256k1_voi_amd 0.4 (gfx950)"; }
#define S2K_STR2(x) #x
#define S2K_STR(x) S2K_STR2(x)
#ifndef S2K_BUILD_FLAGS
#define S2K_BUILD_FLAGS ""
#endif
const char* s2k_build_config(void) {
  return "GT_BITS=" S2K_STR(S2K_GT_BITS) " GT_BITS_FIRST=" S2K_STR(S2K_GT_BITS_FIRST) " PREP_M=" S2K_STR(S2K_PREP_M)
         " QT_PACK=" S2K_STR(S2K_QT_PACK) " FAST_WAVES=" S2K_STR(S2K_FAST_WAVES) " STRIDE_PAD=" S2K_STR(S2K_STRIDE_PAD)
         " ROW_MAX=" S2K_STR(S2K_ROW_MAX_DEFAULT) " QUAD_MAX=" S2K_STR(S2K_QUAD_MAX_DEFAULT) " COMB_LEAD=" S2K_STR(S2K_COMB_LEAD_DEFAULT)
         " flags=[" S2K_BUILD_FLAGS "]";
}
const char* s2k_last_error(const s2k_ctx* ctx) { return ctx ? ctx->err : g_err; }
int s2k_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}
// "0000:05:00.0" of a device (hipDeviceGetPCIBusId): what topology.cpp looks up in sysfs
int s2k_device_pci_bus_id(int device, char* out, size_t len) {
  if (!out || len < 13) return S2K_ERR_ARG;
  out[0] = 0;
  if (hipDeviceGetPCIBusId(out, (int)len, device) != hipSuccess) {
    (void)hipGetLastError();
    out[0] = 0;
    return S2K_ERR_NO_DEVICE;
  }
  return S2K_OK;
}

// workspace (32-bit words per lane, lane stride = n rounded up to 64):
//   [0,256)    per-lane point table of the fast path: 8 entries x 8 quads (tb_*); the complete path
//              uses the first 192 words for its projective table
//   [256,304)  four scratch field elements ("fin": X, Y, Z for k_affine_finish; Z_7*C / prefix products)
//   then       17 words of scalar-prep output, 36 words for the generator part (grouped flow).  The prep kernel's own scratch (prefix products and
//              s in Montgomery form, 10 words each) borrows the start of the table region,
//              which is only written after the prep kernel has finished.
//   then       worklist: 1 counter + n indices
constexpr size_t WS_QT = 0, WS_FIN = TBL_WORDS, WS_PREP = TBL_WORDS + FIN_WORDS, WS_PREF = WS_QT, WS_SMONT = WS_QT + 10,
                 WS_GP = WS_PREP + PREP_WORDS, WS_LANE_WORDS = WS_GP + 3 * FQT_FE_WORDS;
static_assert(TBL_WORDS >= QT_WORDS, "the complete path's table must fit in the fast path's region");
}  // extern "C"
__attribute__((visibility("hidden"))) lane_ws lane_ws_of(const s2k_ctx* ctx, size_t n) {
  const size_t stride = lane_stride(n);
  uint32_t* ws = (uint32_t*)ctx->ws;
  lane_ws w;
  w.qt = ws + WS_QT * stride;
  w.fin = ws + WS_FIN * stride;
  w.prep = ws + WS_PREP * stride;
  w.gp = ws + WS_GP * stride;
  w.pref = ws + WS_PREF * stride;
  w.smont = ws + WS_SMONT * stride;
  w.wl_count = ws + WS_LANE_WORDS * stride;
  w.wl = w.wl_count + 64;
  w.stride = stride;
  return w;
}
extern "C" {

size_t s2k_ecdsa_workspace_bytes(size_t n) {
  return (lane_stride(n) * WS_LANE_WORDS + 64 + lane_stride(n)) * sizeof(uint32_t);
}
size_t s2k_ctx_device_bytes(const s2k_ctx* ctx, size_t n) {
  if (!ctx) return 0;
  size_t total = s2k_ecdsa_workspace_bytes(n);
  {
    uint64_t info[4] = {0, 0, 0, 0};
    (void)s2k_ctx_gt_info(const_cast<s2k_ctx*>(ctx), info);
    total += (size_t)info[3] + (info[2] ? gt_bytes_of((int)info[1]) : 0);   // the tables held, and the one being built
  }
  if (ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH) total += s2k_internal_key_bytes(ctx, n);
  return total;
}

// (shared with ops.hip; not part of the ABI)
__attribute__((visibility("hidden"))) int s2k_internal_ensure_ws(s2k_ctx* ctx, size_t n) {
  size_t need = s2k_ecdsa_workspace_bytes(n);
  if (need <= ctx->ws_bytes) return S2K_OK;
  if (ctx->ws) {
    HIP_TRY(ctx, hipFree(ctx->ws));
    ctx->ws = nullptr;
    ctx->ws_bytes = 0;
    ctx->last_wl_count = nullptr;   // pointed into the old workspace (s2k_ctx_key_grouping_stats)
  }
  HIP_TRY(ctx, hipMalloc(&ctx->ws, need));
  ctx->ws_bytes = need;
  return S2K_OK;
}

namespace {
std::atomic<size_t> g_keyset_budget{0};           // s2k_set_table_memory_budgets: what counts as free for a key set's joint tables (0: what is free)
}  // namespace
// (pointset.hip: a point set's tables count against the same cap as a key set's joint tables)
__attribute__((visibility("hidden"))) size_t s2k_internal_keyset_budget() { return g_keyset_budget.load(); }

extern "C" {
// Caps on the two other table kinds, per process (0 = none): what s2k_keyset_create_ex treats as free memory when it chooses or
// checks a joint-table layout, and the largest per-key table buffer a verification call may allocate (larger requests are
// treated as failed allocations: the table cap halves, below 1024 tables the batch is verified without tables).  These replace
// the S2K_TEST_* environment variables of round 4 (no ambient test hooks in allocation paths).
void s2k_set_table_memory_budgets(size_t keyset_free_bytes, size_t key_table_bytes) {
  g_keyset_budget.store(keyset_free_bytes);
  s2k_internal_key_table_limit().store(key_table_bytes);
}
}  // extern "C"

int s2k_ctx_create(int device_index, s2k_ctx** out) { return s2k_ctx_create_ex(device_index, 0, 0, out); }

// gt_bits: 0 = automatic (above); 16 .. 26 = exactly that window width for this context's generator tables, built before the
// call returns.  flags: S2K_CTX_WAIT_TABLES = return only when the background build has ended (a context that must run at
// full speed from its first call: benchmarks).
int s2k_ctx_create_ex(int device_index, int gt_bits, uint32_t flags, s2k_ctx** out) {
  if (!out) return fail(nullptr, S2K_ERR_ARG, "s2k_ctx_create: out is NULL");
  *out = nullptr;
  if (gt_bits != 0 && (gt_bits < 16 || gt_bits > GT_BITS_MAX)) return fail(nullptr, S2K_ERR_ARG, "generator window width %d: 0 (automatic) or 16 .. %d", gt_bits, GT_BITS_MAX);
  if (flags & ~(uint32_t)S2K_CTX_WAIT_TABLES) return fail(nullptr, S2K_ERR_ARG, "unknown context flags");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(nullptr, S2K_ERR_NO_DEVICE, "no HIP device visible (this engine has no CPU fallback)");
  if (device_index < 0 || device_index >= count)
    return fail(nullptr, S2K_ERR_ARG, "device index %d out of range (0..%d)", device_index, count - 1);
  s2k_ctx* ctx = new (std::nothrow) s2k_ctx();
  if (!ctx) return fail(nullptr, S2K_ERR_NOMEM, "out of host memory");
  ctx->device = device_index;
  {
    static std::atomic<uint64_t> next_generation{1};
    ctx->generation = next_generation.fetch_add(1);
  }
  if (getrandom(&ctx->kg_seed, sizeof ctx->kg_seed, 0) != (ssize_t)sizeof ctx->kg_seed) ctx->kg_seed = 0x5ec9u;   // hash seed of the key grouping
  if (const char* v = getenv("S2K_KEYED_PARTS")) {        // measurement knob: 2 = the two-part flow (grouped_front)
    int np = atoi(v);
    if (np == 1 || np == 2) ctx->kg_parts = (uint32_t)np;
  }
  if (const char* v = getenv("S2K_KEYED_LADDER")) {       // "window": the ECDSA and BIP-340 calls of this context build 16-bit chunk tables (s2k_ctx_set_keyed_ladder)
    if (!strcmp(v, "window")) ctx->kt_comb = false;
  }
  if (const char* v = getenv("S2K_GP_FIRST_PERCENT")) {   // measurement knob (tools/keyed_probe.py)
    int pc = atoi(v);
    if (pc >= 0 && pc <= 100) ctx->gp_first_percent = (uint32_t)pc;
  }
  hipError_t e = hipSetDevice(device_index);
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device_index);
  if (e == hipSuccess) ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->clk, 64);
  if (e == hipSuccess) e = hipMemset(ctx->clk, 0, 64);
  if (e == hipSuccess) {
    e = s2k_internal_gt_acquire(device_index, gt_bits);
    if (e == hipSuccess) {
      ctx->gt_held = true;
      ctx->gt_fixed = gt_bits;
    } else if (e == hipErrorOutOfMemory) {
      (void)fail(nullptr, S2K_ERR_NOMEM, "context creation failed: no device memory for the %d-bit generator tables (%.1f GiB)",
                 gt_bits ? gt_bits : GT_BITS_FIRST, gt_bytes_of(gt_bits ? gt_bits : GT_BITS_FIRST) / 1073741824.0);
    }
  }
  if (e != hipSuccess) {
    int rc = e == hipErrorOutOfMemory ? S2K_ERR_NOMEM : fail(nullptr, S2K_ERR_HIP, "context creation failed: %s", hipGetErrorString(e));
    if (ctx->clk) (void)hipFree(ctx->clk);
    if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
    delete ctx;
    return rc;
  }
  if (flags & S2K_CTX_WAIT_TABLES) (void)s2k_ctx_gt_wait(ctx);
  *out = ctx;
  return S2K_OK;
}

void s2k_ctx_destroy(s2k_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (s2k_ctx::pipe_slot& sl : ctx->pipe) {          // batches still in flight are waited for (their verdicts are delivered)
    if (sl.ctx) {
      (void)s2k_internal_pipe_retire(ctx, sl);
      s2k_ctx_destroy(sl.ctx);
      sl.ctx = nullptr;
    }
    if (sl.h_valid) (void)hipHostFree(sl.h_valid);
    sl.h_valid = nullptr;
    if (sl.done) (void)hipEventDestroy(sl.done);
    sl.done = nullptr;
    for (hipEvent_t* e : {&sl.t_begin, &sl.t_copied, &sl.t_end}) {
      if (*e) (void)hipEventDestroy(*e);
      *e = nullptr;
    }
  }
  if (ctx->kga_note) {                                // (a kernel still in flight may hold the address)
    (void)hipDeviceSynchronize();
    (void)hipHostFree(ctx->kga_note);
  }
  if (ctx->gt_held) s2k_internal_gt_release(ctx->device);
  if (ctx->ws) (void)hipFree(ctx->ws);
  if (ctx->msm_ws) (void)hipFree(ctx->msm_ws);
  if (ctx->seg_ws) (void)hipFree(ctx->seg_ws);
  if (ctx->seg_host) (void)hipHostFree(ctx->seg_host);
  if (ctx->h2c_dev) (void)hipFree(ctx->h2c_dev);
  if (ctx->h2c_host) (void)hipHostFree(ctx->h2c_host);
  if (ctx->rlc_save) (void)hipFree(ctx->rlc_save);
  if (ctx->msg_digest) (void)hipFree(ctx->msg_digest);
  if (ctx->rec_keys) (void)hipFree(ctx->rec_keys);
  if (ctx->io) (void)hipFree(ctx->io);
  if (ctx->h_small) (void)hipHostFree(ctx->h_small);
  if (ctx->clk) (void)hipFree(ctx->clk);
  if (ctx->ev_done) (void)hipEventDestroy(ctx->ev_done);
  if (ctx->s_aux && !ctx->streams_shared) (void)hipStreamDestroy(ctx->s_aux);
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->ev_mid) (void)hipEventDestroy(ctx->ev_mid);
  for (hipEvent_t& e : ctx->ev_arrival)
    if (e) (void)hipEventDestroy(e);
  if (ctx->ev_part0) (void)hipEventDestroy(ctx->ev_part0);
  if (ctx->ev_part1) (void)hipEventDestroy(ctx->ev_part1);
  if (ctx->s_aux2) (void)hipStreamDestroy(ctx->s_aux2);
  if (ctx->s_msm_tail) (void)hipStreamDestroy(ctx->s_msm_tail);
  if (ctx->kg) (void)hipFree(ctx->kg);
  if (ctx->ktab) (void)hipFree(ctx->ktab);
  if (ctx->xkeys) (void)hipFree(ctx->xkeys);
  if (ctx->ks_found) (void)hipFree(ctx->ks_found);
  if (ctx->ek_ctr) (void)hipFree(ctx->ek_ctr);
  for (size_t i = 0; i < ctx->prof_cap; ++i) (void)hipEventDestroy(ctx->prof_ev[i]);
  for (size_t i = 0; i < ctx->msm_prof_cap; ++i) (void)hipEventDestroy(ctx->msm_prof_ev[i]);
  delete[] ctx->msm_prof_ev;
  delete[] ctx->prof_ev;
  for (hipEvent_t e : ctx->ev_copied)
    if (e) (void)hipEventDestroy(e);
  if (ctx->lane1_comp) (void)hipStreamDestroy(ctx->lane1_comp);
  if (ctx->lane1_aux) (void)hipStreamDestroy(ctx->lane1_aux);
  if (ctx->s_copy && !ctx->streams_shared) (void)hipStreamDestroy(ctx->s_copy);
  if (ctx->s_comp && !ctx->streams_shared) (void)hipStreamDestroy(ctx->s_comp);
  delete ctx;
}

int s2k_ctx_profile(s2k_ctx* ctx, int enable) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (enable && !ctx->prof_ev) {
    const size_t cap = PROF_EV * 1024;   // 1024 verification calls between two reads
    ctx->prof_ev = new (std::nothrow) hipEvent_t[cap];
    if (!ctx->prof_ev) return fail(ctx, S2K_ERR_NOMEM, "out of host memory");
    for (size_t i = 0; i < cap; ++i) {
      hipError_t e = hipEventCreate(&ctx->prof_ev[i]);
      if (e != hipSuccess) {
        for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(ctx->prof_ev[j]);
        delete[] ctx->prof_ev;
        ctx->prof_ev = nullptr;
        return fail(ctx, S2K_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
      }
    }
    ctx->prof_cap = cap;
  }
  ctx->prof_on = enable != 0;
  ctx->prof_used = 0;
  return S2K_OK;
}

int s2k_ctx_profile_read_stages(s2k_ctx* ctx, double* ms_sum5, double* ms_fast_each, size_t cap, size_t* calls,
                                double* shader_mhz) {
  if (!ctx || !ms_sum5 || !calls) return fail(ctx, S2K_ERR_ARG, "null argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  for (int j = 0; j < PROF_EV - 1; ++j) ms_sum5[j] = 0.0;
  const size_t k = ctx->prof_used / PROF_EV;
  for (size_t i = 0; i < k; ++i) {
    for (int j = 0; j < PROF_EV - 1; ++j) {
      float ms = 0.f;
      HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->prof_ev[PROF_EV * i + j], ctx->prof_ev[PROF_EV * i + j + 1]));
      ms_sum5[j] += ms;
      if (j == 2 && ms_fast_each && i < cap) ms_fast_each[i] = ms;
    }
  }
  *calls = k;
  ctx->prof_used = 0;
  if (shader_mhz) {   // [0]: first wave of the last ladder launch, [1]: a wave of its final round
    uint64_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int wall_khz = 0;
    HIP_TRY(ctx, hipMemcpy(h, ctx->clk, sizeof h, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, ctx->device));
    for (int j = 0; j < 2; ++j) {
      const uint64_t* c = h + 4 * j;
      shader_mhz[j] = (c[3] > c[2] && wall_khz > 0) ? (double)(c[1] - c[0]) / (double)(c[3] - c[2]) * (wall_khz * 1e-3) : 0.0;
    }
  }
  return S2K_OK;
}

// the three-stage view: preparation (with grouping and tables) | ladder | everything after it
int s2k_ctx_profile_read(s2k_ctx* ctx, double* ms_sum3, double* ms_fast_each, size_t cap, size_t* calls,
                         double* shader_mhz) {
  if (!ctx || !ms_sum3 || !calls) return fail(ctx, S2K_ERR_ARG, "null argument");
  double s5[5];
  int rc = s2k_ctx_profile_read_stages(ctx, s5, ms_fast_each, cap, calls, shader_mhz);
  if (rc) return rc;
  ms_sum3[0] = s5[0] + s5[1];
  ms_sum3[1] = s5[2];
  ms_sum3[2] = s5[3] + s5[4];
  return S2K_OK;
}

// `arrivals` (optional): d_dig / d_r / d_s become valid piece by piece - signatures [lo[c], lo[c] + cnt[c]) after event
// ev[c]; the keys (d_pub) are valid in stream order.  The host-buffer entry point copies the keys first and lets the
// grouping and the per-key tables - which need nothing else - start while the rest of the batch is still crossing PCIe;
// the scalar preparation and the generator part of a piece follow its arrival on the second stream.
struct sig_arrivals {
  int count;
  size_t lo[8], cnt[8];
  hipEvent_t ev[8];
};
static int verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r, const void* d_s,
                               uint32_t flags, void* d_valid, void* hip_stream, const sig_arrivals* arrivals);
int s2k_ecdsa_verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r,
                                  const void* d_s, uint32_t flags, void* d_valid, void* hip_stream) {
  return verify_batch_device(ctx, n, d_pub, d_dig, d_r, d_s, flags, d_valid, hip_stream, nullptr);
}
static int verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pub, const void* d_dig, const void* d_r, const void* d_s,
                               uint32_t flags, void* d_valid, void* hip_stream, const sig_arrivals* arrivals) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_pub || !d_dig || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  const lane_ws w = lane_ws_of(ctx, n);
  const uint8_t *pub = (const uint8_t*)d_pub, *dig = (const uint8_t*)d_dig, *r = (const uint8_t*)d_r, *s = (const uint8_t*)d_s;
  uint8_t* valid = (uint8_t*)d_valid;
  ctx->kg_counters = nullptr;
  ctx->last_wl_count = nullptr;
  ctx->kt_last = -1;
  auto wait_all = [&](hipStream_t on) {
    if (arrivals)
      for (int c = 0; c < arrivals->count; ++c) (void)hipStreamWaitEvent(on, arrivals->ev[c], 0);
  };
  if (flags & S2K_ECDSA_FORCE_COMPLETE) {
    wait_all(st);
    launch_ecdsa_verify(ctx, st, n, w, pub, dig, r, s, flags, valid);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  const uint32_t T = prep_lanes(n);
  const uint32_t kvf = (flags & S2K_ECDSA_FORCE_WORKLIST) ? KVF_FORCE_WORKLIST : 0u;
  uint64_t* clk = ctx->prof_on ? ctx->clk : nullptr;
  bool grouped = ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH;
  // small batches: a wave per signature beats any table (k_verify_row); a grouping mode somebody asked for by name
  // (S2K_KEYS_AUTO / S2K_KEYS_ALWAYS) is obeyed instead
  const bool row = n <= ctx->row_max && !kvf && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  // ... and up to quad_max four lanes per signature (k_verify_quad): half the latency of the lane kernels for calls that fill
  // neither
  const bool quad = !row && n <= ctx->quad_max && !kvf && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  if (row || quad) grouped = false;
  else HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));      // (these ladders have no worklist: one launch less)
  ctx->kg_note_dst = nullptr;
  if (grouped && ctx->kg_mode == S2K_KEYS_ADAPTIVE && n >= KG_ADAPT_MIN_BATCH) grouped = kg_adaptive_decide(ctx);
  if (grouped) {
    // the grouping arrays and the table buffer, before anything of this call is in flight; a device without room for the
    // tables verifies without them
    rc = s2k_internal_key_reserve(ctx, n, 64);
    if (rc == S2K_ERR_NOMEM) grouped = false;
    else if (rc) return rc;
  }
  ctx->last_wl_count = (row || quad) ? nullptr : w.wl_count;
  prof_mark(ctx, st, 0);
  if (grouped) {
    // Signatures of keys that occur often enough: per-key tables (keyed.hip) and the short ladder; the
    // rest: the general kernel over the list `left`.
    key_groups kg;
    ctx->kt_comb_call = ctx->kt_comb;
    rc = grouped_front(ctx, st, n, pub, 64, w,
                       [&](hipStream_t aux) {
                         if (!arrivals) {
                           launch_scalar_prep(aux, w, 0, n, T, dig, r, s, nullptr, flags);
                           return;
                         }
                         // piece by piece: the planes of the workspace are linear in the signature index, so a piece is
                         // the same kernels on shifted pointers
                         for (int c = 0; c < arrivals->count; ++c) {
                           const size_t lo = arrivals->lo[c], cnt = arrivals->cnt[c];
                           (void)hipStreamWaitEvent(aux, arrivals->ev[c], 0);
                           launch_scalar_prep(aux, w, lo, cnt, prep_lanes(cnt), dig, r, s, nullptr, flags);
                           launch_generator_part(ctx, aux, w, (uint32_t)lo, (uint32_t)(lo + cnt));
                         }
                       },
                       &kg, /*gp_in_prep=*/arrivals != nullptr);
    ctx->kt_comb_call = false;
    if (rc) return rc;
    ctx->kt_last = kg.chunks == KC_TEETH ? S2K_LADDER_COMB : S2K_LADDER_WINDOW;
    prof_mark(ctx, st, 2);
    // the ladder of the tables the grouping built: the comb's, or the window ladder over the 16-bit chunks
    const int keyed_mode = kg.chunks == KC_TEETH ? MODE_ECDSA_COMB : MODE_ECDSA_KEYED;
    launch_ladder(ctx, st, keyed_mode, n, kvf, pub, r, w, valid, nullptr, clk, kg);
    HIP_TRY(ctx, hipGetLastError());
    if (kg.nparts > 1) {   // the other side of the split, once its tables (third stream) are there
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_part1, 0));
      kg.part = 1;
      launch_ladder(ctx, st, keyed_mode, n, kvf, pub, r, w, valid, nullptr, nullptr, kg);
      HIP_TRY(ctx, hipGetLastError());
    }
    prof_mark(ctx, st, 3);
    launch_ladder(ctx, st, MODE_ECDSA_LEFT, n, kvf, pub, r, w, valid, nullptr, nullptr, kg);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 4);
  } else if (quad) {
    // four lanes per signature on the complete formulas (k_verify_quad), behind a preparation with one lane per signature
    wait_all(st);
    launch_scalar_prep(st, w, 0, n, (uint32_t)n, dig, r, s, nullptr, flags);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_verify_quad(ctx, st, n, pub, r, w, valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else if (row) {
    // small batches: a wave per signature on the complete formulas (k_verify_row); nothing is left for the worklist kernel
    wait_all(st);
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_verify_row(ctx, st, n, pub, dig, r, s, flags, valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else {
    wait_all(st);
    launch_scalar_prep(st, w, 0, n, T, dig, r, s, nullptr, flags);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_ladder(ctx, st, MODE_ECDSA, n, kvf, pub, r, w, valid, nullptr, clk, key_groups{});
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
  }
  if (ctx->dbg_gt_swap) {   // test hook: the wide table appears HERE, between the ladder and the kernel that finishes its tagged lanes
    const int bits = ctx->dbg_gt_swap;
    ctx->dbg_gt_swap = 0;
    HIP_TRY(ctx, s2k_internal_gt_debug_publish(ctx->device, bits));
#ifdef S2K_DEBUG_GT_PER_LAUNCH   // (variant build that restores the fault of round 5 - a view per launch - to show the test sees it)
    ctx->gt_call = s2k_internal_gt_load(ctx);
#endif
  }
  launch_verify_fallback(ctx, st, n, w, pub, dig, r, s, flags, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

int s2k_ctx_set_key_grouping(s2k_ctx* ctx, int mode, uint32_t min_group, uint32_t hash_bits, uint32_t max_tables) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (mode != S2K_KEYS_OFF && mode != S2K_KEYS_AUTO && mode != S2K_KEYS_ALWAYS && mode != S2K_KEYS_ADAPTIVE)
    return fail(ctx, S2K_ERR_ARG, "key grouping mode %d", mode);
  if (hash_bits > 30) return fail(ctx, S2K_ERR_ARG, "hash_bits %u > 30", hash_bits);
  ctx->kg_mode = mode;
  ctx->kg_min_group = min_group;
  ctx->kg_hash_bits = hash_bits;
  ctx->kg_max_tables = max_tables ? max_tables : KG_MAX_TABLES_DEFAULT;
  ctx->kg_table_cap = 0;           // (a cap found by an earlier allocation failure is tried afresh)
  return S2K_OK;
}

int s2k_ctx_set_keyed_ladder(s2k_ctx* ctx, int ladder) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (ladder != S2K_LADDER_COMB && ladder != S2K_LADDER_WINDOW) return fail(ctx, S2K_ERR_ARG, "keyed ladder %d", ladder);
  ctx->kt_comb = ladder == S2K_LADDER_COMB;
  return S2K_OK;
}

int s2k_ctx_last_keyed_ladder(s2k_ctx* ctx) { return ctx ? ctx->kt_last : -1; }
int s2k_ctx_last_keyset_ladder(s2k_ctx* ctx) { return ctx ? ctx->ks_last : -1; }

int s2k_ctx_key_grouping_stats(s2k_ctx* ctx, uint32_t* stats) {
  if (!ctx || !stats) return fail(ctx, S2K_ERR_ARG, "null argument");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  if (ctx->kg_counters) {
    uint32_t c[KG_COUNTERS];
    HIP_TRY(ctx, hipMemcpy(c, ctx->kg_counters, sizeof c, hipMemcpyDeviceToHost));
    stats[0] = c[KG_NKEYED];
    stats[1] = c[KG_NTAB] < ctx->kg_last_max_tables ? c[KG_NTAB] : ctx->kg_last_max_tables;
    stats[2] = c[KG_NLEFT];
  }
  if (ctx->last_wl_count) HIP_TRY(ctx, hipMemcpy(&stats[3], ctx->last_wl_count, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return S2K_OK;
}

int s2k_ctx_key_grouping_adaptive(s2k_ctx* ctx, uint32_t* out, int reset) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (out) {
    out[0] = ctx->kga_miss_streak;
    out[1] = ctx->kga_miss_streak >= KG_ADAPT_MISSES ? ctx->kga_skip_left : 0;
    out[2] = ctx->kga_skipped;
    out[3] = ctx->kga_probes;
    out[4] = ctx->kga_observed;
  }
  if (reset) {
    ctx->kga_miss_streak = ctx->kga_skip_left = 0;
    ctx->kga_skipping = false;
    ctx->kga_seen = ctx->kga_seq;                      // notes still on their way are not taken
  }
  return S2K_OK;
}

int s2k_ecdsa_recover_batch_device(s2k_ctx* ctx, size_t n, const void* d_dig, const void* d_r, const void* d_s,
                                   const void* d_recid, uint32_t flags, void* d_pub65, void* d_ok, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_dig || !d_r || !d_s || !d_recid || !d_pub65 || !d_ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  const lane_ws w = lane_ws_of(ctx, n);
  const uint8_t *dig = (const uint8_t*)d_dig, *r = (const uint8_t*)d_r, *s = (const uint8_t*)d_s,
                *rid = (const uint8_t*)d_recid;
  uint8_t *ok = (uint8_t*)d_ok, *pub65 = (uint8_t*)d_pub65;
  if (flags & S2K_ECDSA_FORCE_COMPLETE) {
    launch_recover_fallback(ctx, st, n, w, dig, r, s, rid, ok, pub65);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  // (stage times, s2k_ctx_profile_read_stages: [0] the scalar preparation, [2] the ladder, [3] the shared inversions of the
  // affine results, [4] the worklist)
  prof_mark(ctx, st, 0);
  if (n <= ctx->row_max) {
    // small batches: a wave per item, one launch (k_recover_row: preparation, ladder, inversion and record)
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_recover_row(ctx, st, n, dig, r, s, rid, ok, pub65);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  }
  if (n <= ctx->quad_max) {
    // four lanes per item (k_recover_quad) between a preparation and a finish with one lane per item
    launch_scalar_prep(st, w, 0, n, (uint32_t)n, dig, r, s, rid, 0u);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemsetAsync(d_pub65, 0, n * 65, st));      // items without a key keep the zero record
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_recover_quad(ctx, st, n, r, w, ok);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    launch_affine_finish(st, MODE_RECOVER, n, (uint32_t)n, nullptr, w, ok, pub65);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  }
  HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));
  launch_scalar_prep(st, w, 0, n, prep_lanes(n), dig, r, s, rid, 0u);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemsetAsync(d_pub65, 0, n * 65, st));      // items without a key keep the zero record
  prof_mark(ctx, st, 1);
  prof_mark(ctx, st, 2);
  launch_ladder(ctx, st, MODE_RECOVER, n, 0u, nullptr, r, w, ok, pub65, ctx->prof_on ? ctx->clk : nullptr, key_groups{});
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 3);
  launch_affine_finish(st, MODE_RECOVER, n, (uint32_t)((n + FIN_M - 1) / FIN_M), nullptr, w, ok, pub65);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  launch_recover_worklist(ctx, st, n, w, dig, r, s, rid, ok, pub65);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

int s2k_ecdsa_recover_batch(s2k_ctx* ctx, size_t n, const uint8_t* dig, const uint8_t* r, const uint8_t* s,
                            const uint8_t* recid, uint32_t flags, uint8_t* pub65, uint8_t* ok) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!dig || !r || !s || !recid || !pub65 || !ok) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const stage_part parts[6] = {stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_in(recid, n), stage_out(pub65, n * 65), stage_out(ok, n)};
  return s2k_internal_staged_call(ctx, parts, 6, n * 97, s2k_internal_small_call(ctx, n, flags), [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_recover_batch_device(c, n, d[0], d[1], d[2], d[3], flags, d[4], d[5], st);
  });
}

int s2k_schnorr_verify_batch_device(s2k_ctx* ctx, size_t n, const void* d_pk, const void* d_msgs,
                                    const void* d_msg_offsets, size_t msg_len, const void* d_sig, uint32_t flags,
                                    void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!d_pk || !d_sig || !d_valid || (!d_msgs && (d_msg_offsets || msg_len)))
    return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  const lane_ws w = lane_ws_of(ctx, n);
  const uint8_t* pk = (const uint8_t*)d_pk;
  const uint8_t* sig = (const uint8_t*)d_sig;
  const uint8_t* msgs = (const uint8_t*)d_msgs;
  const uint64_t* offs = (const uint64_t*)d_msg_offsets;
  const uint32_t mlen = (uint32_t)msg_len;
  uint8_t* valid = (uint8_t*)d_valid;
  if (flags & S2K_ECDSA_FORCE_COMPLETE) {
    launch_schnorr_fallback(ctx, st, n, w, pk, sig, msgs, offs, mlen, valid);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  // (stage times, s2k_ctx_profile_read_stages: [0] the front end - challenge hashes, and the grouping and per-key tables when
  // keys repeat -, [2] the ladder over per-key tables or the general one, [3] what the key tables left + the shared inversions,
  // [4] the worklist)
  prof_mark(ctx, st, 0);
  ctx->kg_counters = nullptr;
  ctx->kt_last = -1;
  bool grouped = ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH;
  const bool row = n <= ctx->row_max && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  const bool quad = !row && n <= ctx->quad_max && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF);
  if (row || quad) grouped = false;
  else HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));
  ctx->last_wl_count = (row || quad) ? nullptr : w.wl_count;
  if (grouped) {
    rc = s2k_internal_key_reserve(ctx, n, 32);
    if (rc == S2K_ERR_NOMEM) grouped = false;      // no room for per-key tables: the general ladder for everything
    else if (rc) return rc;
  }
  if (grouped) {
    // signatures that share an x-only key: the grouped flow of the ECDSA path (s2k_ctx_set_key_grouping)
    key_groups kg;
    ctx->kt_comb_call = ctx->kt_comb;
    rc = grouped_front(ctx, st, n, pk, 32, w, [&](hipStream_t aux) { launch_schnorr_prep(aux, n, w, pk, sig, msgs, offs, mlen); }, &kg);
    ctx->kt_comb_call = false;
    if (rc) return rc;
    ctx->kt_last = kg.chunks == KC_TEETH ? S2K_LADDER_COMB : S2K_LADDER_WINDOW;
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    // the ladder of the tables the grouping built: the comb's, or the window ladder over the 16-bit chunks
    const int keyed_mode = kg.chunks == KC_TEETH ? MODE_SCHNORR_COMB : MODE_SCHNORR_KEYED;
    launch_ladder(ctx, st, keyed_mode, n, 0u, pk, sig, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, kg);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    if (kg.nparts > 1) {
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_part1, 0));
      kg.part = 1;
      launch_ladder(ctx, st, keyed_mode, n, 0u, pk, sig, w, valid, nullptr, nullptr, kg);
      HIP_TRY(ctx, hipGetLastError());
    }
    launch_ladder(ctx, st, MODE_SCHNORR_LEFT, n, 0u, pk, sig, w, valid, nullptr, nullptr, kg);
    HIP_TRY(ctx, hipGetLastError());
  } else if (quad) {
    // four lanes per signature (k_schnorr_quad) behind the preparation kernel; nothing left for the finish and worklist kernels
    launch_schnorr_prep(st, n, w, pk, sig, msgs, offs, mlen);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_schnorr_quad(ctx, st, n, pk, sig, w, valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else if (row) {
    // small batches: a wave per signature, nothing left for the finish and worklist kernels (k_schnorr_row): one launch up to
    // 1024 signatures, the preparation kernel in front above
    if (n <= 1024) {
      prof_mark(ctx, st, 1);
      prof_mark(ctx, st, 2);
      launch_schnorr_row(ctx, st, n, pk, sig, msgs, offs, mlen, nullptr, 0, valid);
    } else {
      launch_schnorr_prep(st, n, w, pk, sig, msgs, offs, mlen);
      HIP_TRY(ctx, hipGetLastError());
      prof_mark(ctx, st, 1);
      prof_mark(ctx, st, 2);
      launch_schnorr_row(ctx, st, n, pk, sig, msgs, offs, mlen, w.prep, w.stride, valid);
    }
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  } else {
    launch_schnorr_prep(st, n, w, pk, sig, msgs, offs, mlen);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    launch_ladder(ctx, st, MODE_SCHNORR, n, 0u, pk, sig, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, key_groups{});
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
  }
  launch_affine_finish(st, MODE_SCHNORR, n, (uint32_t)((n + FIN_M - 1) / FIN_M), sig, w, valid, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  launch_schnorr_worklist(ctx, st, n, w, pk, sig, msgs, offs, mlen, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

// Host-buffer entry point.  The batch is cut into chunks that are whole rounds of k_verify_fast
// on this device (3 waves/SIMD x 4 SIMDs x CUs x 64 lanes; one round first, then two per chunk), and the
// host-to-device copy of chunk j+1 runs on its own stream while chunk j is verified: for pageable
// callers' memory the copy costs about half as much as the verification, so most of it hides.
// Staging buffers and streams live in the context (no hipMalloc per call).
// Everything of a host-buffer verification except the final wait: copies in, kernels, verdicts to h_out (host memory; the
// copy is asynchronous when h_out is page-locked).  All work ends on ctx->s_comp.  one_shot: the batch is not cut into
// chunks (submit / wait: the other slot's batch is what this one's transfer hides behind, and ONE grouped call sees every
// signature of a key).  On an error nothing of the call is left in flight.
static int verify_batch_enqueue_inner(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                      const uint8_t* s, uint32_t flags, uint8_t* h_out, bool one_shot) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  rc = ctx_reserve(ctx, &ctx->io, &ctx->io_bytes, n * 161 + 1024);
  if (rc) return rc;
  uint8_t* d_pub = (uint8_t*)ctx->io;
  uint8_t* d_dig = d_pub + n * 64;
  uint8_t* d_r = d_dig + n * 32;
  uint8_t* d_s = d_r + n * 32;
  uint8_t* d_valid = d_s + n * 32;
  // Pinned host buffers (s2k_host_alloc / s2k_host_register, or the caller's own hipHostMalloc): copies are truly
  // asynchronous, so with the grouping on the whole batch goes through ONE grouped call - the keys are copied first, the
  // grouping and the per-key tables start on them, and the digests and signatures cross PCIe meanwhile (the scalar
  // preparation on the second stream waits for them).  From pageable memory a copy is staged by the runtime and the
  // same order measured slower than two independent halves (9.0 against 8.4-8.6 ms per 2^20), which stay the path there.
  const bool pinned = s2k_internal_host_pinned(pub, n * 64) && s2k_internal_host_pinned(dig, n * 32) && s2k_internal_host_pinned(r, n * 32) &&
                      s2k_internal_host_pinned(s, n * 32);
  // (submit / wait, one_shot: no pieces - the other tickets' kernels are what the transfer hides behind, and the ticket runs
  // one compute stream; measured 5.07 against 5.13 ms per 2^20 with the pieces.  S2K_SUBMIT_ARRIVALS=1: measurement knob)
  static const bool submit_arrivals = [] { const char* v = getenv("S2K_SUBMIT_ARRIVALS"); return v && atoi(v) != 0; }();
  if (pinned && ctx->kg_mode != S2K_KEYS_OFF && n >= KG_MIN_BATCH && (!one_shot || submit_arrivals)) {
    rc = ctx_arrival_events(ctx);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_pub, pub, n * 64, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_copied[0], ctx->s_copy));
    sig_arrivals arr;
    arr.count = n >= ((size_t)1 << 16) ? 4 : 1;
    const size_t per = ((n + arr.count - 1) / arr.count + 255) & ~(size_t)255;
    for (int c = 0; c < arr.count; ++c) {
      const size_t lo = (size_t)c * per, cnt = lo >= n ? 0 : (n - lo < per ? n - lo : per);
      arr.lo[c] = lo;
      arr.cnt[c] = cnt;
      arr.ev[c] = ctx->ev_arrival[c];
      if (cnt) {
        HIP_TRY(ctx, hipMemcpyAsync(d_r + lo * 32, r + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
        HIP_TRY(ctx, hipMemcpyAsync(d_s + lo * 32, s + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
        HIP_TRY(ctx, hipMemcpyAsync(d_dig + lo * 32, dig + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
      }
      HIP_TRY(ctx, hipEventRecord(arr.ev[c], ctx->s_copy));
    }
    while (arr.count > 1 && arr.cnt[arr.count - 1] == 0) --arr.count;
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_comp, ctx->ev_copied[0], 0));
    rc = verify_batch_device(ctx, n, d_pub, d_dig, d_r, d_s, flags, d_valid, ctx->s_comp, &arr);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(h_out, d_valid, n, hipMemcpyDeviceToHost, ctx->s_comp));
    return S2K_OK;
  }
  const size_t round = (size_t)S2K_FAST_WAVES * 4 * (size_t)ctx->cu_count * 64;
  // chunks are whole rounds of the ladder kernel; the first one is a single round, because its copy is
  // the only one nothing hides (63 -> 31 MB up front at 256 CUs), the others two rounds
  const bool chunked = !one_shot && n > 3 * round;         // small batches: one shot
  // with key grouping on, every chunk groups (and builds tables) on its own, so fewer and larger chunks:
  // two halves, the second copy hidden behind the first half's kernels
  const bool halves = chunked && ctx->kg_mode != S2K_KEYS_OFF;
  int k = 0;
  for (size_t lo = 0, chunk = 0; lo < n; lo += chunk, ++k) {
    chunk = !chunked ? n : halves ? ((n / 2 + 255) & ~(size_t)255) : (lo == 0 ? round : 2 * round);
    if (n - lo < chunk + round) chunk = n - lo;            // no launch of less than a round at the end
    const size_t cnt = chunk;
    // the event of two chunks ago has been waited on by s_comp (in stream order) before it is re-recorded
    HIP_TRY(ctx, hipMemcpyAsync(d_pub + lo * 64, pub + lo * 64, cnt * 64, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipMemcpyAsync(d_dig + lo * 32, dig + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipMemcpyAsync(d_r + lo * 32, r + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipMemcpyAsync(d_s + lo * 32, s + lo * 32, cnt * 32, hipMemcpyHostToDevice, ctx->s_copy));
    HIP_TRY(ctx, hipEventRecord(ctx->ev_copied[k & 1], ctx->s_copy));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_comp, ctx->ev_copied[k & 1], 0));
    rc = s2k_ecdsa_verify_batch_device(ctx, cnt, d_pub + lo * 64, d_dig + lo * 32, d_r + lo * 32, d_s + lo * 32, flags,
                                       d_valid + lo, ctx->s_comp);
    if (rc) return rc;
  }
  HIP_TRY(ctx, hipMemcpyAsync(h_out, d_valid, n, hipMemcpyDeviceToHost, ctx->s_comp));
  return S2K_OK;
}
static int verify_batch_enqueue(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                const uint8_t* s, uint32_t flags, uint8_t* h_out, bool one_shot) {
  const int rc = verify_batch_enqueue_inner(ctx, n, pub, dig, r, s, flags, h_out, one_shot);
  if (rc) s2k_internal_drain(ctx);
  return rc;
}

int s2k_ecdsa_verify_batch(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                           const uint8_t* s, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!pub || !dig || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  int rc;
  if (s2k_internal_small_call(ctx, n, flags) && (ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF)) {
    // (ctx_small_block: the wave-per-signature ladder reads the caller's bytes from page-locked memory and writes the verdicts
    // there - no DMA transfers)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    rc = ctx_streams(ctx);
    if (rc) return rc;
    const size_t sizes[5] = {n * 64, n * 32, n * 32, n * 32, n};
    uint8_t *h[5], *d[5];
    rc = s2k_internal_small_block(ctx, sizes, 5, h, d);
    if (rc) return rc;
    memcpy(h[0], pub, n * 64);
    memcpy(h[1], dig, n * 32);
    memcpy(h[2], r, n * 32);
    memcpy(h[3], s, n * 32);
    rc = s2k_ecdsa_verify_batch_device(ctx, n, d[0], d[1], d[2], d[3], flags, d[4], ctx->s_comp);
    if (rc) {
      s2k_internal_drain(ctx);
      return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->s_comp));
    memcpy(valid, h[4], n);
    return S2K_OK;
  }
  rc = verify_batch_enqueue(ctx, n, pub, dig, r, s, flags, valid, /*one_shot=*/false);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->s_comp));
  return S2K_OK;
}

int s2k_ecdsa_verify_batch_submit(s2k_ctx* ctx, size_t n, const uint8_t* pub, const uint8_t* dig, const uint8_t* r,
                                  const uint8_t* s, uint32_t flags, uint8_t* valid, s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  if (n && (!pub || !dig || !r || !s || !valid)) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  s2k_ctx::pipe_slot* sl = nullptr;
  int rc = s2k_internal_pipe_slot(ctx, n, valid, &sl);
  if (rc) return rc;
  if (n) {
    rc = verify_batch_enqueue(sl->ctx, n, pub, dig, r, s, flags, sl->direct ? valid : sl->h_valid, /*one_shot=*/true);
    if (rc) return fail(ctx, rc, "%s", sl->ctx->err);
  }
  s2k_internal_pipe_issue(ctx, sl, ticket);
  return S2K_OK;
}

// Batches of up to max_n signatures take the wave-per-signature ladder (k_verify_row); 0 switches it off.
int s2k_ctx_set_small_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->row_max = max_n;
  return S2K_OK;
}
// ECDSA batches above that and up to max_n take the four-lanes-per-signature ladder (k_verify_quad); 0 switches it off.
// Key-set calls of up to max_n signatures take the wave-per-signature ladder over the set's tables (k_verify_row_keyset /
// k_schnorr_row_keyset); 0 switches it off.  Comb sets have the threshold below.
int s2k_ctx_set_keyset_small_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->ks_row_max = max_n;
  return S2K_OK;
}
// ... and over a COMB set (k_verify_row_comb / k_schnorr_row_comb), a threshold of its own: 0, the default, is never
int s2k_ctx_set_keyset_comb_small_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->ks_comb_row_max = max_n;
  return S2K_OK;
}
int s2k_ctx_set_mid_batch_max(s2k_ctx* ctx, uint32_t max_n) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->quad_max = max_n;
  return S2K_OK;
}

int s2k_schnorr_verify_batch(s2k_ctx* ctx, size_t n, const uint8_t* pk, const uint8_t* msgs,
                             const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig, uint32_t flags,
                             uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!pk || !sig || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const size_t total = msg_offsets ? (size_t)msg_offsets[n] : n * msg_len, off_bytes = (n + 1) * sizeof(uint64_t);
  if (total && !msgs) return fail(ctx, S2K_ERR_ARG, "null message buffer");
  const stage_part parts[5] = {stage_in(pk, n * 32), stage_in(msgs, total, total ? total : 16), stage_in(msg_offsets, msg_offsets ? off_bytes : 0, off_bytes),
                               stage_in(sig, n * 64), stage_out(valid, n)};
  const bool small = s2k_internal_small_call(ctx, n, flags) && total <= ((size_t)1 << 20);
  return s2k_internal_staged_call(ctx, parts, 5, n * 96 + total, small, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_schnorr_verify_batch_device(c, n, d[0], d[1], msg_offsets ? d[2] : nullptr, msg_len, d[3], flags, d[4], st);
  });
}

// Point.DoubleScalarMultBasepointVartime (point_mul_glv.go:307), or scalarMultVartimeGLV (:203) when
// u1 == NULL, over a batch of 65-byte records; host pointers.  impl selects the arithmetic (header).
int s2k_double_scalar_mult_basepoint_batch_ex(s2k_ctx* ctx, uint32_t impl, size_t n, const uint8_t* u1, const uint8_t* u2,
                                              const uint8_t* points, uint8_t* out) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (impl != S2K_IMPL_COMPLETE && impl != S2K_IMPL_FAST) return fail(ctx, S2K_ERR_ARG, "unknown implementation selector");
  if (n == 0) return S2K_OK;
  if (!u2 || !points || !out) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  hipStream_t st = ctx->s_comp;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_u1 = 0, o_u2 = pad(n * 32), o_pts = o_u2 + pad(n * 32), o_out = o_pts + pad(n * 65), o_pub = o_out + pad(n * 65),
               o_ok = o_pub + pad(n * 64), o_status = o_ok + pad(n);
  rc = ctx_reserve(ctx, &ctx->io, &ctx->io_bytes, o_status + 256);
  if (rc) return rc;
  uint8_t* io = (uint8_t*)ctx->io;
  if (u1)
    HIP_TRY(ctx, hipMemcpyAsync(io + o_u1, u1, n * 32, hipMemcpyHostToDevice, st));
  else
    HIP_TRY(ctx, hipMemsetAsync(io + o_u1, 0, n * 32, st));   // plain scalar multiplication: u1 = 0
  HIP_TRY(ctx, hipMemcpyAsync(io + o_u2, u2, n * 32, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(io + o_pts, points, n * 65, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(io + o_status, 0, 4, st));
  const uint8_t* d_u1 = io + o_u1;
  const lane_ws w = lane_ws_of(ctx, n);
  uint32_t* status = (uint32_t*)(io + o_status);
  if (impl == S2K_IMPL_COMPLETE) {
    launch_point_fallback(ctx, st, /*all=*/true, n, w, d_u1, io + o_u2, io + o_pts, io + o_out, status);
    HIP_TRY(ctx, hipGetLastError());
  } else {
    HIP_TRY(ctx, hipMemsetAsync(w.wl_count, 0, sizeof(uint32_t), st));
    HIP_TRY(ctx, hipMemsetAsync(io + o_out, 0, n * 65, st));   // (the ladder kernel leaves the records of undecided lanes alone)
    launch_hot_prep(st, n, w, d_u1, io + o_u2, io + o_pts, io + o_pub, status);
    HIP_TRY(ctx, hipGetLastError());
    launch_ladder(ctx, st, MODE_POINT, n, 0u, io + o_pub, nullptr, w, io + o_ok, io + o_out, nullptr, key_groups{});
    HIP_TRY(ctx, hipGetLastError());
    launch_affine_finish(st, MODE_RECOVER, n, (uint32_t)((n + FIN_M - 1) / FIN_M), nullptr, w, io + o_ok, io + o_out);
    HIP_TRY(ctx, hipGetLastError());
    launch_point_fallback(ctx, st, /*all=*/false, n, w, d_u1, io + o_u2, io + o_pts, io + o_out, status);
    HIP_TRY(ctx, hipGetLastError());
  }
  uint32_t h_status = 0;
  HIP_TRY(ctx, hipMemcpyAsync(out, io + o_out, n * 65, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(&h_status, status, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  if (h_status) return fail(ctx, S2K_ERR_ARG, "malformed point record (not an encoding the reference's Point can hold)");
  return S2K_OK;
}

}  // extern "C"
