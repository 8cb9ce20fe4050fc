// pipeline.hip — how host arrays reach a device form and come back, for every entry point that takes host pointers (host code
// only; engine.hip, keyset.hip, digest.hip and ingest.hip call it through engine_internal.h): page-locked memory
// (s2k_host_*), the page-locked block of small synchronous calls, staging around a device form (s2k_internal_staged_call /
// _staged_submit), and the tickets of submit / wait - slots, lanes, s2k_wait / s2k_poll / s2k_wait_all and their timing.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <unistd.h>

#include "engine_internal.h"

// Small synchronous calls from host memory (up to the small-batch threshold, s2k_ctx_set_small_batch_max): the inputs are
// copied by the CPU into a page-locked block that the kernels read in place, and the kernels write the results there - no
// DMA transfer at all.  The five transfers of a 1024-signature call cost 45 us of its 0.23 ms, more than its 160 KB take
// either way.  `count` pieces of `sizes[i]` bytes, 256-byte aligned; host[i] / dev[i]: the same piece as the CPU and as the
// device address it.  (Synchronous entry points only: the block is free again when the call returns.)
__attribute__((visibility("hidden"))) int s2k_internal_small_block(s2k_ctx* ctx, const size_t* sizes, int count, uint8_t** host, uint8_t** dev) {
  size_t total = 0;
  for (int i = 0; i < count; ++i) total += (sizes[i] + 255) & ~(size_t)255;
  if (total > ctx->h_small_bytes) {
    if (ctx->h_small) (void)hipHostFree(ctx->h_small);
    ctx->h_small = ctx->d_small = nullptr;
    ctx->h_small_bytes = 0;
    const size_t want = (total + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1);
    void *h = nullptr, *d = nullptr;
    HIP_TRY(ctx, hipHostMalloc(&h, want, hipHostMallocDefault));
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipHostFree(h);
      return fail(ctx, S2K_ERR_HIP, "hipHostGetDevicePointer failed for the small-call block");
    }
    ctx->h_small = (uint8_t*)h;
    ctx->d_small = (uint8_t*)d;
    ctx->h_small_bytes = want;
  }
  size_t off = 0;
  for (int i = 0; i < count; ++i) {
    host[i] = ctx->h_small + off;
    dev[i] = ctx->d_small + off;
    off += (sizes[i] + 255) & ~(size_t)255;
  }
  return S2K_OK;
}
__attribute__((visibility("hidden"))) bool s2k_internal_small_call(const s2k_ctx* ctx, size_t n, uint32_t flags) {
  static const bool off = [] { const char* v = getenv("S2K_SMALL_CALLS_DMA"); return v && atoi(v) != 0; }();   // (A/B knob)
  return !off && n <= ctx->row_max && !(flags & (S2K_ECDSA_FORCE_COMPLETE | S2K_ECDSA_FORCE_WORKLIST));
}

// page-locked host memory the runtime can copy from asynchronously (hipHostMalloc or hipHostRegister)
static bool host_pinned_at(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();          // an ordinary malloc'ed pointer: "invalid value", not an error of ours
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
// (first AND last byte: a buffer registered for fewer bytes than the call reads must not take the asynchronous path)
static bool host_pinned(const void* p, size_t bytes) {
  return host_pinned_at(p) && (bytes < 2 || host_pinned_at((const uint8_t*)p + bytes - 1));
}
extern "C" {
void* s2k_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}
void s2k_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}
int s2k_host_register(void* p, size_t bytes) {
  if (!p || !bytes) return fail(nullptr, S2K_ERR_ARG, "s2k_host_register: null buffer");
  // Whole pages only.  The runtime pins and, on unregister, unmaps PAGES: registering a block of the C heap takes the
  // neighbouring blocks of its first and last page along.  Seen on ROCm 7.2 / MI355X: four small malloc'ed arrays
  // registered and unregistered, the allocator hands the same pages out again as part of a 2 MB block, and a plain
  // pageable hipMemcpy from that block dies with a GPU memory access fault (tests/test_gpu_round3.py history).
  const size_t page = (size_t)sysconf(_SC_PAGESIZE);
  if (((uintptr_t)p % page) || (bytes % page))
    return fail(nullptr, S2K_ERR_ARG, "s2k_host_register: buffer must start on a page boundary and cover whole pages (%zu bytes): "
                                      "register memory that owns its pages (mmap, aligned_alloc), or use s2k_host_alloc", page);
  hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, S2K_ERR_HIP, "hipHostRegister: %s", hipGetErrorString(e));
  }
  return S2K_OK;
}
int s2k_host_unregister(void* p) {
  if (!p) return fail(nullptr, S2K_ERR_ARG, "s2k_host_unregister: null buffer");
  hipError_t e = hipHostUnregister(p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, S2K_ERR_HIP, "hipHostUnregister: %s", hipGetErrorString(e));
  }
  return S2K_OK;
}
}  // extern "C"

// An error return leaves copies from (and to) caller-owned memory in flight on the context's streams: wait for them before the
// caller may free or unregister that memory (the message of the error is kept).
__attribute__((visibility("hidden"))) void s2k_internal_drain(s2k_ctx* ctx) {
  if (ctx->s_copy) (void)hipStreamSynchronize(ctx->s_copy);
  if (ctx->s_aux) (void)hipStreamSynchronize(ctx->s_aux);
  if (ctx->s_comp) (void)hipStreamSynchronize(ctx->s_comp);
  (void)hipGetLastError();
}

// ---------------------------------------------------------------------------------------
// submit / wait: the host-pointer entry points without the wait at their end.  The reference's caller holds its data in
// host memory (secec/ecdsa.go:171-228) and a synchronous call pays transfer and compute in series: 7.1 ms from pinned
// memory, 8.2 from pageable against 4.9 ms resident per 2^20 signatures (round 3).  Here the context owns child contexts
// ("slots": own workspaces and staging buffers; the 40 GiB generator tables are shared per device) that take the submitted
// batches in turn.  The children run on the PARENT's streams, in two lanes: even tickets on the parent's own two compute
// streams, odd tickets on a second pair, one copy stream for all.  Within a lane the kernels of consecutive tickets follow
// each other in stream order, each ticket with the two-stream overlap of a resident call (grouping and tables beside
// preparation and generator part); the lanes run beside each other as two resident contexts do (worth 3 %); a ticket's
// 160 MiB cross PCIe (3.0 ms) on the copy stream beside the kernels of the tickets before it.  Up to four tickets are in
// flight (per lane one computing, one arriving); a fifth submit first retires the oldest one (its verdicts are delivered;
// a later s2k_wait on its ticket returns at once).
// (Earlier forms gave every ticket streams of its own so that one ticket's grouping and tables could run beside another's
// ladder.  They do not: the keyed ladder holds 4 x 128 of a SIMD's 512 VGPRs, so the other ticket's kernels crawl, its
// empty tail launches - 161 VGPRs a wave - wait milliseconds for room, and nine streams on the runtime's hardware queues
// serialise at random.  5.2-5.7 ms per batch against 4.7-4.9 this way; profiles/r04_pipeline_timeline.txt.)
// ---------------------------------------------------------------------------------------
static void pipe_note_failure(s2k_ctx* ctx, uint64_t ticket, int rc) {
  const unsigned i = ctx->pipe_failed_n++ % 8u;
  ctx->pipe_failed[i] = ticket;
  ctx->pipe_failed_rc[i] = rc;
}
// waits for the slot's batch and delivers its verdicts; the slot is free afterwards
__attribute__((visibility("hidden"))) int s2k_internal_pipe_retire(s2k_ctx* ctx, s2k_ctx::pipe_slot& sl) {
  if (!sl.ticket) return S2K_OK;
  int rc = S2K_OK;
  if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(sl.done) != hipSuccess) {
    rc = fail(ctx, S2K_ERR_HIP, "ticket %llu: the batch did not complete: %s", (unsigned long long)sl.ticket,
              hipGetErrorString(hipGetLastError()));
    s2k_internal_drain(sl.ctx);
  } else if (!sl.direct) {
    memcpy(sl.dst, sl.h_valid, sl.n);
  }
  if (rc == S2K_OK && sl.timed) {                    // s2k_ctx_ticket_timing: transfer and whole-ticket time on the device's clock
    float h2d = 0, all = 0;
    // (t_copied sits on the copy stream behind the ticket's transfers; with more streams in the process than hardware queues
    // its marker can still be waiting in a shared queue when the ticket's verdicts are there - eight members on one device
    // showed it: then it is waited for, the copies themselves are long done)
    const hipError_t e0 = hipEventSynchronize(sl.t_end);
    hipError_t e1 = hipEventElapsedTime(&h2d, sl.t_begin, sl.t_copied);
    if (e1 == hipErrorNotReady) {
      (void)hipGetLastError();
      (void)hipEventSynchronize(sl.t_copied);
      e1 = hipEventElapsedTime(&h2d, sl.t_begin, sl.t_copied);
    }
    const hipError_t e2 = hipEventElapsedTime(&all, sl.t_begin, sl.t_end);
    const unsigned i = ctx->pipe_times_n++ % 8u;
    ctx->pipe_times_ticket[i] = sl.ticket;
    if (e0 == hipSuccess && e1 == hipSuccess && e2 == hipSuccess) {
      ctx->pipe_times_ms[i][0] = h2d;
      ctx->pipe_times_ms[i][1] = all;
    } else {                                           // no times for this ticket: the runtime's codes, negated, say why
      (void)hipGetLastError();
      ctx->pipe_times_ms[i][0] = -(float)(e1 != hipSuccess ? e1 : e0);
      ctx->pipe_times_ms[i][1] = -(float)(e2 != hipSuccess ? e2 : e0);
    }
  }
  sl.timed = false;
  sl.ticket = 0;
  return rc;
}
// the slot the next ticket runs on, free, with its child context and landing buffer in place
__attribute__((visibility("hidden"))) int s2k_internal_pipe_slot(s2k_ctx* ctx, size_t n, uint8_t* valid, s2k_ctx::pipe_slot** out) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  s2k_ctx::pipe_slot& sl = ctx->pipe[ctx->pipe_next % s2k_ctx::PIPE_SLOTS];
  if (sl.ticket) {                                   // every slot holds a batch: the oldest one (this slot's) is retired first
    const uint64_t t = sl.ticket;
    const int rc = s2k_internal_pipe_retire(ctx, sl);
    if (rc) pipe_note_failure(ctx, t, rc);           // (reported by s2k_wait on that ticket)
  }
  if (!sl.ctx) {
    // first use of the slot.  All or nothing: a failure anywhere leaves the slot as it was found (no child context, no
    // event), so that the next submit tries again from the start instead of running on a half-built slot.
    int rc = ctx_streams(ctx);                        // the parent's three streams carry every ticket
    if (rc == S2K_OK) rc = ctx_aux_streams(ctx);
    if (rc) return rc;
    const bool odd_lane = (ctx->pipe_next & 1u) != 0;   // (PIPE_SLOTS is even: a slot always serves the same lane)
    static const bool one_lane = [] { const char* v = getenv("S2K_SUBMIT_ONE_LANE"); return v && atoi(v) != 0; }();   // measurement knob
    if (odd_lane && !one_lane && !(ctx->lane1_comp && ctx->lane1_aux)) {   // the second lane's two streams: both or neither
      hipStream_t a = nullptr, b = nullptr;
      if (hipStreamCreateWithFlags(&a, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&b, hipStreamNonBlocking) != hipSuccess) {
        const hipError_t e = hipGetLastError();
        if (a) (void)hipStreamDestroy(a);
        if (b) (void)hipStreamDestroy(b);
        return fail(ctx, S2K_ERR_HIP, "submit: streams of the second lane: %s", hipGetErrorString(e));
      }
      ctx->lane1_comp = a;
      ctx->lane1_aux = b;
    }
    s2k_ctx* child = nullptr;
    rc = s2k_ctx_create_ex(ctx->device, ctx->gt_fixed, 0, &child);   // the parent's table width, explicit or automatic
    if (rc) return fail(ctx, rc, "submit: child context: %s", s2k_last_error(nullptr));
    child->s_copy = ctx->s_copy;
    child->s_comp = (odd_lane && !one_lane) ? ctx->lane1_comp : ctx->s_comp;
    child->s_aux = (odd_lane && !one_lane) ? ctx->lane1_aux : ctx->s_aux;
    child->streams_shared = true;
    rc = ctx_streams(child);                          // (its events)
    if (rc == S2K_OK) rc = ctx_aux_streams(child);
    hipEvent_t done = nullptr;
    if (rc == S2K_OK && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) {
      snprintf(child->err, sizeof child->err, "hipEventCreate: %s", hipGetErrorString(hipGetLastError()));
      rc = S2K_ERR_HIP;
    }
    if (rc) {
      rc = fail(ctx, rc, "submit: child context: %s", child->err);
      s2k_ctx_destroy(child);                         // (streams_shared: the parent's streams stay)
      return rc;
    }
    sl.ctx = child;
    sl.done = done;
  }
  if (ctx->pipe_timing && !sl.t_begin) {              // timing events on demand; a failure only means no times for this slot
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    bool ok = true;
    for (int i = 0; i < 3 && ok; ++i) ok = hipEventCreate(&e[i]) == hipSuccess;
    if (ok) {
      sl.t_begin = e[0];
      sl.t_copied = e[1];
      sl.t_end = e[2];
    } else {
      (void)hipGetLastError();
      for (int i = 0; i < 3; ++i)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  }
  sl.timed = ctx->pipe_timing && sl.t_begin && hipEventRecord(sl.t_begin, ctx->s_copy) == hipSuccess;
  // the child verifies with the parent's settings of the moment
  sl.ctx->kg_mode = ctx->kg_mode;
  sl.ctx->parent = ctx;
  sl.ctx->kg_min_group = ctx->kg_min_group;
  sl.ctx->kg_hash_bits = ctx->kg_hash_bits;
  sl.ctx->kg_max_tables = ctx->kg_max_tables;
  sl.ctx->kt_comb = ctx->kt_comb;
  sl.ctx->row_max = ctx->row_max;
  sl.ctx->ks_row_max = ctx->ks_row_max;
  sl.ctx->ks_comb_row_max = ctx->ks_comb_row_max;
  sl.ctx->quad_max = ctx->quad_max;
  sl.direct = host_pinned(valid, n);
  if (!sl.direct && sl.h_valid_bytes < n) {
    if (sl.h_valid) (void)hipHostFree(sl.h_valid);
    sl.h_valid = nullptr;
    sl.h_valid_bytes = 0;
    const size_t want = (n + 4095) & ~(size_t)4095;
    HIP_TRY(ctx, hipHostMalloc((void**)&sl.h_valid, want, hipHostMallocDefault));
    sl.h_valid_bytes = want;
  }
  sl.dst = valid;
  sl.n = n;
  *out = &sl;
  return S2K_OK;
}
__attribute__((visibility("hidden"))) void s2k_internal_pipe_issue(s2k_ctx* ctx, s2k_ctx::pipe_slot* sl, s2k_ticket* ticket) {
  // s2k_ctx_ticket_timing: t_begin (s2k_internal_pipe_slot) and t_copied bracket the ticket's transfers on the copy stream; the
  // compute stream WAITS for t_copied before t_end is recorded behind the verdicts, so that first copy start <= last copy end
  // <= verdicts holds on the device's clock however the runtime multiplexes the streams onto hardware queues (eight members on
  // one device: a marker could be processed after another stream's later one).  Costs the ticket nothing
  // while the timing is off.
  if (sl->timed)
    sl->timed = hipEventRecord(sl->t_copied, ctx->s_copy) == hipSuccess && hipStreamWaitEvent(sl->ctx->s_comp, sl->t_copied, 0) == hipSuccess &&
                hipEventRecord(sl->t_end, sl->ctx->s_comp) == hipSuccess;
  if (hipEventRecord(sl->done, sl->ctx->s_comp) != hipSuccess) {    // behind the ticket's last operation (on its lane's stream)
    // no event to wait on: the ticket is made to finish here, so that s2k_wait finds it done (or reports this failure)
    const hipError_t e = hipGetLastError();
    (void)hipStreamSynchronize(sl->ctx->s_comp);
    (void)fail(ctx, S2K_ERR_HIP, "submit: hipEventRecord: %s", hipGetErrorString(e));
  }
  sl->ticket = ctx->pipe_next++;
  *ticket = sl->ticket;
}
__attribute__((visibility("hidden"))) bool s2k_internal_host_pinned(const void* p, size_t bytes) { return host_pinned(p, bytes); }

// Staging around a device form (engine_internal.h: stage_part).  The inputs of a call up, on `st` ...
static int stage_copies_in(s2k_ctx* ctx, const stage_part* parts, int count, uint8_t* const* d, hipStream_t st) {
  for (int i = 0; i < count; ++i)
    if (parts[i].src && parts[i].bytes) HIP_TRY(ctx, hipMemcpyAsync(d[i], parts[i].src, parts[i].bytes, hipMemcpyHostToDevice, st));
  return S2K_OK;
}
// ... and its results back (landing: where a ticket's verdicts go instead of the caller's array; null: to the parts' own dst)
static int stage_copies_out(s2k_ctx* ctx, const stage_part* parts, int count, uint8_t* const* d, hipStream_t st, void* landing) {
  for (int i = 0; i < count; ++i)
    if (parts[i].dst) HIP_TRY(ctx, hipMemcpyAsync(landing ? landing : parts[i].dst, d[i], parts[i].bytes, hipMemcpyDeviceToHost, st));
  return S2K_OK;
}
__attribute__((visibility("hidden"))) int s2k_internal_staged_call(s2k_ctx* ctx, const stage_part* parts, int count, size_t phase_bytes,
                                                                   bool small, const stage_run& run) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  size_t sizes[STAGE_MAX_PARTS];
  uint8_t *h[STAGE_MAX_PARTS], *d[STAGE_MAX_PARTS];
  for (int i = 0; i < count; ++i) sizes[i] = parts[i].reserve;
  hipStream_t st = ctx->s_comp;
  if (small) {                                             // (s2k_internal_small_block: no DMA transfers)
    rc = s2k_internal_small_block(ctx, sizes, count, h, d);
    if (rc) return rc;
    for (int i = 0; i < count; ++i)
      if (parts[i].src && parts[i].bytes) memcpy(h[i], parts[i].src, parts[i].bytes);
    rc = run(ctx, d, st);
    if (rc) {
      s2k_internal_drain(ctx);
      return rc;
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < count; ++i)
      if (parts[i].dst) memcpy(parts[i].dst, h[i], parts[i].bytes);
    ctx->have_last = false;
    return S2K_OK;
  }
  // staged in the context's buffers on its compute stream (no allocation per call)
  rc = ctx_stage(ctx, sizes, count, d);
  if (rc) return rc;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  s2k_phase_guard phase(ctx->device, phase_bytes);         // (two verifiers on two threads: engine_internal.h)
  rc = stage_copies_in(ctx, parts, count, d, st);
  if (rc) return rc;
  HIP_TRY(ctx, phase.landed(st));
  rc = run(ctx, d, st);
  if (rc) {
    s2k_internal_drain(ctx);
    return rc;
  }
  rc = stage_copies_out(ctx, parts, count, d, st, nullptr);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(st));
  ctx->have_last = false;
  return S2K_OK;
}
__attribute__((visibility("hidden"))) int s2k_internal_staged_submit(s2k_ctx* ctx, size_t n, uint8_t* valid, const stage_part* parts, int count,
                                                                     const stage_run& run, s2k_ticket* ticket) {
  s2k_ctx::pipe_slot* sl = nullptr;
  int rc = s2k_internal_pipe_slot(ctx, n, valid, &sl);
  if (rc) return rc;
  if (n) {
    s2k_ctx* c = sl->ctx;
    auto enqueue = [&]() -> int {
      size_t sizes[STAGE_MAX_PARTS];
      uint8_t* d[STAGE_MAX_PARTS];
      for (int i = 0; i < count; ++i) sizes[i] = parts[i].reserve;
      int rc2 = ctx_stage(c, sizes, count, d);
      if (rc2 == S2K_OK) rc2 = stage_copies_in(c, parts, count, d, c->s_copy);
      if (rc2) return rc2;
      HIP_TRY(c, hipEventRecord(c->ev_copied[0], c->s_copy));
      HIP_TRY(c, hipStreamWaitEvent(c->s_comp, c->ev_copied[0], 0));
      rc2 = run(c, d, c->s_comp);
      if (rc2) return rc2;
      return stage_copies_out(c, parts, count, d, c->s_comp, sl->direct ? valid : sl->h_valid);
    };
    rc = enqueue();
    if (rc) {
      s2k_internal_drain(c);
      return fail(ctx, rc, "%s", c->err);
    }
  }
  s2k_internal_pipe_issue(ctx, sl, ticket);
  return S2K_OK;
}

extern "C" {
int s2k_wait(s2k_ctx* ctx, s2k_ticket ticket) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (ticket == 0 || ticket >= ctx->pipe_next) return fail(ctx, S2K_ERR_ARG, "s2k_wait: ticket %llu was never issued", (unsigned long long)ticket);
  for (s2k_ctx::pipe_slot& sl : ctx->pipe)
    if (sl.ticket == ticket) return s2k_internal_pipe_retire(ctx, sl);
  for (unsigned i = 0; i < 8; ++i)                    // retired by a later submit: its verdicts are delivered (or it failed then)
    if (ctx->pipe_failed[i] == ticket) return fail(ctx, ctx->pipe_failed_rc[i], "ticket %llu failed when it was retired", (unsigned long long)ticket);
  return S2K_OK;
}

// S2K_OK: the ticket's verdicts are delivered (as s2k_wait); S2K_PENDING: still in flight.  Never blocks.
int s2k_poll(s2k_ctx* ctx, s2k_ticket ticket) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (ticket == 0 || ticket >= ctx->pipe_next) return fail(ctx, S2K_ERR_ARG, "s2k_poll: ticket %llu was never issued", (unsigned long long)ticket);
  for (s2k_ctx::pipe_slot& sl : ctx->pipe)
    if (sl.ticket == ticket) {
      HIP_TRY(ctx, hipSetDevice(ctx->device));
      const hipError_t e = hipEventQuery(sl.done);
      if (e == hipErrorNotReady) {
        (void)hipGetLastError();
        return S2K_PENDING;
      }
      return s2k_internal_pipe_retire(ctx, sl);
    }
  return s2k_wait(ctx, ticket);                       // retired earlier
}

int s2k_wait_all(s2k_ctx* ctx) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = S2K_OK;
  for (;;) {                                          // oldest first
    s2k_ctx::pipe_slot* oldest = nullptr;
    for (s2k_ctx::pipe_slot& sl : ctx->pipe)
      if (sl.ticket && (!oldest || sl.ticket < oldest->ticket)) oldest = &sl;
    if (!oldest) break;
    const int r1 = s2k_internal_pipe_retire(ctx, *oldest);
    if (r1 && !rc) rc = r1;
  }
  return rc;
}

// Per-ticket times on the device's clock (for placement diagnostics, s2k_group_member_stats_ex): enable, submit, wait, ask.
int s2k_ctx_ticket_timing(s2k_ctx* ctx, int enable) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  ctx->pipe_timing = enable != 0;
  return S2K_OK;
}
int s2k_ticket_times(s2k_ctx* ctx, s2k_ticket ticket, double ms[2]) {
  if (!ctx || !ms) return fail(ctx, S2K_ERR_ARG, "null argument");
  for (unsigned i = 0; i < 8; ++i)
    if (ticket && ctx->pipe_times_ticket[i] == ticket) {
      ms[0] = ctx->pipe_times_ms[i][0];
      ms[1] = ctx->pipe_times_ms[i][1];
      return S2K_OK;
    }
  ms[0] = ms[1] = 0;
  return S2K_PENDING;      // not retired yet, timing was off, or more than eight tickets ago
}
}  // extern "C"
