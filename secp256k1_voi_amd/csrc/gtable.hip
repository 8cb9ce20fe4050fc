// gtable.hip — the resident generator tables: the two kernels that build them, the per-device registry with its
// background builder, and the s2k_ctx_gt_* entry points.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "engine_internal.h"
#include "fe.h"
#include "point.h"

using namespace s2k;

// ---------------------------------------------------------------------------------------
// Generator tables, resident in HBM:  GT_WINDOWS = ceil(256 / GT_BITS) tables of 2^GT_BITS affine
// points (64 MiB at 16 bits, 3 GiB at 22, 11 GiB at 24, 40 GiB at 26: the default),
//   T_0[d] = d * G - sum_{i>=1} B_i,   T_i[d] = (d + 1) * B_i,   B_i = 2^(GT_BITS i) * G,
// so that  u*G = sum_i T_i[(u >> GT_BITS i) & mask]  with GT_WINDOWS mixed additions, no
// doublings, no zero-digit special case (no entry is the identity) and no final correction.
// The reference's scalarBaseMultVartime (point_mul_table.go:197-211) is the same idea with
// 8-bit windows, sized for a CPU cache (510 KiB); HBM capacity buys wider windows here.  At 16
// bits the even-numbered windows of the reference's table blob are entries of these tables
// (tests/golden/gentable.json).
// Entry layout: 16 x u32 = X limbs (little-endian words) then Y limbs, 64-byte aligned.
// ---------------------------------------------------------------------------------------
// bases[i] = B_i = 2^(bits i) G (affine, 16 words) for i < windows; bases[windows] = -sum_{i>=1} B_i
__global__ void k_gen_gtable_bases(uint32_t* __restrict__ bases, uint32_t bits, uint32_t windows) {
  apt g;
  g.x = fe_from_limbs(FE_GX);
  g.y = fe_from_limbs(FE_GY);
  pt cur = pt_from_affine(g), sum = pt_identity();
#pragma unroll 1
  for (uint32_t i = 0; i <= windows; ++i) {
    apt a;
    if (i < windows) {
      pt_to_affine(a, cur);
      if (i >= 1) sum = pt_add_complete(sum, cur);
#pragma unroll 1
      for (uint32_t t = 0; t < bits; ++t) cur = pt_double_complete(cur);
    } else {
      pt_to_affine(a, pt_cond_neg(sum, true));
    }
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      bases[i * 16 + w] = a.x.v[w];
      bases[i * 16 + 8 + w] = a.y.v[w];
    }
  }
}
// one lane per entry: m * B_w by a double-and-add of bits + 1 steps (m = digit, or digit + 1 for w >= 1)
// (block0: the first block of this launch - the background build launches a table window by window)
__global__ void __launch_bounds__(256) k_gen_gtable(uint32_t* __restrict__ gt, const uint32_t* __restrict__ bases, uint32_t bits, uint32_t windows,
                                                    uint32_t block0) {
  size_t id = ((size_t)block0 + blockIdx.x) * 256 + threadIdx.x;
  uint32_t window = (uint32_t)(id >> bits), digit = (uint32_t)id & ((1u << bits) - 1u);
  apt b;
#pragma unroll
  for (int w = 0; w < 8; ++w) {
    b.x.v[w] = bases[window * 16 + w];
    b.y.v[w] = bases[window * 16 + 8 + w];
  }
  uint32_t m = window ? digit + 1 : digit;      // <= 2^bits
  pt acc = pt_identity();
#pragma unroll 1
  for (int bit = (int)bits; bit >= 0; --bit) {
    acc = pt_double_complete(acc);
    pt sum = pt_add_mixed(acc, b);
    acc = pt_select((m >> bit) & 1u, acc, sum);
  }
  if (window == 0) {
    apt c;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      c.x.v[w] = bases[windows * 16 + w];
      c.y.v[w] = bases[windows * 16 + 8 + w];
    }
    acc = pt_add_mixed(acc, c);
  }
  apt a;
  pt_to_affine(a, acc);
  uint4* o = reinterpret_cast<uint4*>(gt + (id << 4));
  o[0] = make_uint4(a.x.v[0], a.x.v[1], a.x.v[2], a.x.v[3]);
  o[1] = make_uint4(a.x.v[4], a.x.v[5], a.x.v[6], a.x.v[7]);
  o[2] = make_uint4(a.y.v[0], a.y.v[1], a.y.v[2], a.y.v[3]);
  o[3] = make_uint4(a.y.v[4], a.y.v[5], a.y.v[6], a.y.v[7]);
}

// The resident generator tables are shared by the contexts of a device (one context per goroutine / thread is the intended
// use): per device one registry with its own lock, reference counted, the last context to go frees it.  A
// registry holds tables of SEVERAL widths:
//   * the first table (GT_BITS_FIRST = 20 bits, 0.8 GiB) is built inside the first s2k_ctx_create: < 0.1 s to a usable context;
//   * an automatic context then starts ONE background thread per device that allocates and builds the wide table
//     (GT_BITS_TARGET = 26 bits / 40 GiB when the device has twice that free and the budget allows, else 24 / 11 GiB, else 22 /
//     3 GiB, else nothing) on a stream of its own, beside whatever the contexts are doing; when it is done, the next CALL of
//     every automatic context uses it (ctx_enter loads the view once; a call never changes tables between its launches).  A
//     failed allocation or build leaves the contexts on the table they have, and is not tried again while the registry lives;
//   * s2k_ctx_create_ex with an explicit width uses exactly that table, built synchronously unless it exists or is being built.
// The builder thread is never detached: the last context to go cancels it (it looks at the flag before it allocates, between
// the windows of a table and before it publishes) and joins it; a process that exits with contexts alive does the same from an
// atexit handler, so that no thread of this library is inside the HIP runtime while that is torn down.
// The reference's analogue is a 510 KiB unpack at package init (point_mul_table.go:75-100).
// (C linkage: g_gtable, gtable_build and the other names of the registry are in the library's dynamic symbol table)
extern "C" {
namespace {
struct gtable_dev {
  std::mutex m;
  std::condition_variable cv;                     // a build has ended (either kind), the builder has been kicked or cancelled
  std::atomic<uint32_t*> table[GT_BITS_MAX + 1];  // by width; non-null = built and readable
  bool being_built[GT_BITS_MAX + 1] = {};         // a thread is building this width outside the lock (others wait for it)
  std::atomic<int> auto_bits{0};                  // width the automatic contexts use now (0: registry empty)
  int refs = 0;
  std::atomic<bool> kicked{false};                // an entry point has enqueued its first call on the device (ctx_leave)
  int target = 0;                                 // width the background build aims for (0: none wanted / none possible)
  bool building = false;                          // the builder thread is running
  bool gave_up = false;                           // a background build failed: not tried again by later contexts of this registry
  bool closing = false;                           // the last context is waiting for the builder to end: nobody acquires meanwhile
  std::atomic<bool> cancel{false};                // the builder is to stop at its next look
  std::atomic<size_t> pending{0};                 // bytes the builder is about to take from the device (s2k_internal_gt_pending_bytes)
  std::thread builder;
  char note[200] = {0};                           // why the target is what it is (s2k_ctx_gt_note; read and written under m)
  gtable_dev() {
    for (auto& t : table) t.store(nullptr);
  }
};
gtable_dev g_gtable[64];
std::atomic<size_t> g_gt_budget{0};               // s2k_set_generator_table_budget: bytes per device the tables may take (0: by free memory)

// allocate and build the table of `bits` on `stream` (null: the default stream); synchronises that stream.  With `cancel` the
// table is built window by window and the flag is looked at in between (hipErrorNotReady: cancelled, nothing is left allocated).
hipError_t gtable_build(int bits, hipStream_t stream, uint32_t** out, const std::atomic<bool>* cancel = nullptr,
                        std::atomic<size_t>* pending = nullptr) {
  const uint32_t windows = gt_windows_of(bits);
  uint32_t *table = nullptr, *bases = nullptr;
  hipError_t e = hipMalloc((void**)&table, gt_bytes_of(bits));
  if (pending) pending->store(0);                 // (taken, or not to be had)
  if (e == hipSuccess) e = hipMalloc((void**)&bases, (windows + 1) * 64);
  if (e == hipSuccess) {
    k_gen_gtable_bases<<<1, 1, 0, stream>>>(bases, (uint32_t)bits, windows);
    const unsigned per_window = (unsigned)(((size_t)1 << bits) / 256);
    if (!cancel) {
      k_gen_gtable<<<per_window * windows, 256, 0, stream>>>(table, bases, (uint32_t)bits, windows, 0u);
      e = hipGetLastError();
    } else {
      for (uint32_t w = 0; w < windows && e == hipSuccess; ++w) {
        if (cancel->load()) {
          e = hipErrorNotReady;
          break;
        }
        k_gen_gtable<<<per_window, 256, 0, stream>>>(table, bases, (uint32_t)bits, windows, w * per_window);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
      }
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  else (void)hipStreamSynchronize(stream);
  if (bases) (void)hipFree(bases);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (table) (void)hipFree(table);
    return e;
  }
  *out = table;
  return hipSuccess;
}

// does a wide table of `bits` fit NOW: twice its size free on the device, so that the tables never take more than half of
// what is left for key sets, workspaces and other processes; and inside the budget.  Asked when the target is chosen and again
// by the builder right before each allocation (half a second or more later).
bool gtable_fits(int bits, size_t* free_out) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (free_out) *free_out = free_b;
  const size_t need = gt_bytes_of(bits), budget = g_gt_budget.load();
  if (budget && need + gt_bytes_of(GT_BITS_FIRST) > budget) return false;
  return free_b >= 2 * need;
}
// the widest of 26 / 24 / 22 (not above `from`, above the first table) that fits; 0: none.  Caller holds g.m (the note).
int gtable_pick_target(gtable_dev& g, int from) {
  size_t free_b = 0;
  const size_t budget = g_gt_budget.load();
  for (int bits : {26, 24, 22}) {
    if (bits > from || bits > GT_BITS_TARGET || bits <= GT_BITS_FIRST) continue;
    if (!gtable_fits(bits, &free_b)) continue;
    snprintf(g.note, sizeof g.note, "%d-bit windows: %.1f GiB of %.1f GiB free%s", bits, gt_bytes_of(bits) / 1073741824.0, free_b / 1073741824.0,
             budget ? " (inside the budget)" : "");
    return bits;
  }
  snprintf(g.note, sizeof g.note, "no wide table fits (%.1f GiB free, budget %.1f GiB): staying on %d bits", free_b / 1073741824.0,
           budget / 1073741824.0, GT_BITS_FIRST);
  return 0;
}

void gtable_builder_main(int device, int bits) {
  gtable_dev& g = g_gtable[device];
  // The allocation of tens of gigabytes holds the runtime's allocator for a second or two, and whatever another thread asks of
  // the runtime meanwhile (its first call's workspace ...) waits behind it: 0.1-0.3 s from s2k_ctx_create to the first verdict
  // became 2.3 s whenever the two collided.  So the build starts when the context's first call has been enqueued (ctx_leave),
  // or after half a second without one.
  {
    std::unique_lock<std::mutex> lock(g.m);
    g.cv.wait_for(lock, std::chrono::milliseconds(500), [&] { return g.kicked.load() || g.cancel.load(); });
  }
  hipError_t e = g.cancel.load() ? hipErrorNotReady : hipSetDevice(device);
  hipStream_t st = nullptr;
  if (e == hipSuccess) {
    int lo = 0, hi = 0;                            // lowest priority: the build yields to verification kernels
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) lo = 0;
    e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, lo);
  }
  const int wanted = bits;
  int built = 0;
  uint32_t* table = nullptr;                       // ours to free unless it is published
  std::unique_lock<std::mutex> lock(g.m);
  while (e == hipSuccess && bits > GT_BITS_FIRST && !g.cancel.load()) {
    if (g.table[bits].load()) {                    // a context with that explicit width built it meanwhile: use that one
      built = bits;
      break;
    }
    if (g.being_built[bits]) {                     // ... or is building it right now: wait for that to end, look again
      g.cv.wait(lock, [&] { return !g.being_built[bits] || g.cancel.load(); });
      continue;
    }
    bits = gtable_pick_target(g, bits);            // (the memory may have gone since the target was chosen)
    if (!bits) break;
    if (g.table[bits].load() || g.being_built[bits]) continue;
    g.being_built[bits] = true;
    g.pending.store(gt_bytes_of(bits));
    lock.unlock();
    const hipError_t be = gtable_build(bits, st, &table, &g.cancel, &g.pending);
    lock.lock();
    g.pending.store(0);
    g.being_built[bits] = false;
    g.cv.notify_all();
    if (be == hipSuccess) {
      built = bits;
      break;
    }
    table = nullptr;
    if (be == hipErrorNotReady) break;             // cancelled
    bits -= 2;                                     // a failed allocation or build: the next width down that fits
  }
  if (g.cancel.load()) {                           // every context went away meanwhile: nobody wants the table
    if (table) (void)hipFree(table);
  } else if (built) {
    if (table && g.table[built].load()) {          // (never two tables of one width: the one that is there stays)
      (void)hipFree(table);
    } else if (table) {
      g.table[built].store(table, std::memory_order_release);
    }
    g.auto_bits.store(built, std::memory_order_release);
    if (built != wanted) snprintf(g.note, sizeof g.note, "%d-bit windows (the table of %d bits could not be had)", built, wanted);
    g.target = built;
  } else {
    if (e != hipSuccess || bits) snprintf(g.note, sizeof g.note, "the wide table could not be built: staying on %d bits", GT_BITS_FIRST);
    g.target = 0;
    g.gave_up = true;
  }
  g.building = false;
  g.cv.notify_all();
  lock.unlock();
  if (st) (void)hipStreamDestroy(st);
}

// a process that exits with contexts alive: the builders are stopped and joined before static destruction and before the HIP
// runtime's own exit handlers (registered earlier than this one, so run later)
void gtable_at_exit() {
  for (gtable_dev& g : g_gtable) {
    std::thread t;
    {
      std::lock_guard<std::mutex> lock(g.m);
      if (!g.builder.joinable()) continue;
      g.cancel.store(true);
      g.cv.notify_all();
      t = std::move(g.builder);
    }
    t.join();
  }
}
}  // namespace
}  // extern "C"

// fixed_bits == 0: the shared automatic tables (first table now, wide table in the background); else exactly that width
__attribute__((visibility("hidden"))) hipError_t s2k_internal_gt_acquire(int device, int fixed_bits) {
  if (device < 0 || device >= 64) return hipErrorInvalidDevice;
  static std::once_flag at_exit_once;
  std::call_once(at_exit_once, [] { (void)atexit(gtable_at_exit); });
  gtable_dev& g = g_gtable[device];
  std::unique_lock<std::mutex> lock(g.m);
  g.cv.wait(lock, [&] { return !g.closing; });    // (the last context of an earlier generation is still joining its builder)
  const int bits = fixed_bits ? fixed_bits : GT_BITS_FIRST;
  while (!g.table[bits].load()) {
    if (g.being_built[bits]) {                     // by the builder or by another context's creation: wait, do not build a second one
      g.cv.wait(lock, [&] { return !g.being_built[bits]; });
      continue;
    }
    g.being_built[bits] = true;
    lock.unlock();                                 // (seconds for a wide table: the contexts of this device keep working)
    uint32_t* t = nullptr;
    const hipError_t e = gtable_build(bits, nullptr, &t);
    lock.lock();
    g.being_built[bits] = false;
    g.cv.notify_all();
    if (e != hipSuccess) return e;
    g.table[bits].store(t, std::memory_order_release);
  }
  if (!fixed_bits) {
    if (g.auto_bits.load() == 0) g.auto_bits.store(GT_BITS_FIRST, std::memory_order_release);
    if (!g.building && !g.gave_up && g.target == 0 && g.auto_bits.load() == GT_BITS_FIRST && GT_BITS_TARGET > GT_BITS_FIRST) {
      g.target = gtable_pick_target(g, GT_BITS_TARGET);
      if (g.target) {
        if (g.table[g.target].load()) {             // (built earlier for a context with that explicit width)
          g.auto_bits.store(g.target, std::memory_order_release);
        } else {
          if (g.builder.joinable()) g.builder.join();   // (an earlier builder that has ended: building is false)
          g.building = true;
          g.cancel.store(false);
          g.pending.store(gt_bytes_of(g.target));
          g.builder = std::thread(gtable_builder_main, device, g.target);
        }
      }
    }
  }
  ++g.refs;
  return hipSuccess;
}
__attribute__((visibility("hidden"))) void s2k_internal_gt_release(int device) {
  gtable_dev& g = g_gtable[device];
  std::unique_lock<std::mutex> lock(g.m);
  if (g.refs <= 0 || --g.refs > 0) return;
  // the last context: stop the builder (it frees what it has not published), wait for it, then free the tables
  g.closing = true;
  g.cancel.store(true);
  g.cv.notify_all();
  std::thread t = std::move(g.builder);
  lock.unlock();
  if (t.joinable()) t.join();
  lock.lock();
  (void)hipSetDevice(device);
  for (auto& tb : g.table) {
    uint32_t* p = tb.exchange(nullptr);
    if (p) (void)hipFree(p);
  }
  g.auto_bits.store(0);
  g.target = 0;
  g.gave_up = false;
  g.building = false;
  g.pending.store(0);
  g.kicked.store(false);
  g.cancel.store(false);
  g.closing = false;
  g.cv.notify_all();
}
__attribute__((visibility("hidden"))) void s2k_internal_gt_kick(int device) {
  gtable_dev& g = g_gtable[device];
  if (g.kicked.load(std::memory_order_relaxed)) return;         // (every call after the first: one relaxed load)
  g.kicked.store(true);
  std::lock_guard<std::mutex> lock(g.m);                        // (so that the notification cannot fall between the builder's test and its wait)
  g.cv.notify_all();
}
// the table a call that starts now uses (ctx_enter: once per call)
__attribute__((visibility("hidden"))) gt_view s2k_internal_gt_load(const s2k_ctx* ctx) {
  const gtable_dev& g = g_gtable[ctx->device];
  const int bits = ctx->gt_fixed ? ctx->gt_fixed : g.auto_bits.load(std::memory_order_acquire);
  gt_view v;
  v.p = g.table[bits].load(std::memory_order_acquire);
  v.bits = (uint32_t)bits;
  v.windows = gt_windows_of(bits);
  return v;
}
// bytes of device memory the background build of this device is about to allocate: whoever sizes something by what is free
// (key-set layouts, the per-key table buffer) takes them off first
__attribute__((visibility("hidden"))) size_t s2k_internal_gt_pending_bytes(int device) {
  return device >= 0 && device < 64 ? g_gtable[device].pending.load() : 0;
}
// Test hook behind s2k_debug_gt_swap_in_call: make `bits` the width of the device's automatic contexts NOW (building the table
// if the registry does not hold it) - what the background builder does at a moment nobody chooses.
__attribute__((visibility("hidden"))) hipError_t s2k_internal_gt_debug_publish(int device, int bits) {
  gtable_dev& g = g_gtable[device];
  std::unique_lock<std::mutex> lock(g.m);
  while (!g.table[bits].load()) {
    if (g.being_built[bits]) {
      g.cv.wait(lock, [&] { return !g.being_built[bits]; });
      continue;
    }
    g.being_built[bits] = true;
    lock.unlock();
    uint32_t* t = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = gtable_build(bits, st, &t);
    if (st) (void)hipStreamDestroy(st);
    lock.lock();
    g.being_built[bits] = false;
    g.cv.notify_all();
    if (e != hipSuccess) return e;
    g.table[bits].store(t, std::memory_order_release);
  }
  g.auto_bits.store(bits, std::memory_order_release);
  return hipSuccess;
}

extern "C" {
// Bytes per device the generator tables of this process may take (0 = no limit but the device's free memory).  Applies to
// automatic contexts created after the call; the first table (0.8 GiB) is always built.
void s2k_set_generator_table_budget(size_t bytes) { g_gt_budget.store(bytes); }
// info[0] = window bits the context's next call uses, [1] = bits the background build aims for (0: none), [2] = 1 while it
// is running, [3] = bytes of generator tables the device holds for this process
int s2k_ctx_gt_info(s2k_ctx* ctx, uint64_t info[4]) {
  if (!ctx || !info) return fail(ctx, S2K_ERR_ARG, "null argument");
  gtable_dev& g = g_gtable[ctx->device];
  std::lock_guard<std::mutex> lock(g.m);
  info[0] = (uint64_t)(ctx->gt_fixed ? ctx->gt_fixed : g.auto_bits.load());
  info[1] = (uint64_t)(ctx->gt_fixed ? 0 : g.target);
  info[2] = g.building && !ctx->gt_fixed ? 1 : 0;
  uint64_t bytes = 0;
  for (int b = GT_BITS_MIN; b <= GT_BITS_MAX; ++b)
    if (g.table[b].load()) bytes += gt_bytes_of(b);
  info[3] = bytes;
  return S2K_OK;
}
// (a copy taken under the lock, owned by the context: the builder thread rewrites the registry's note)
const char* s2k_ctx_gt_note(s2k_ctx* ctx) {
  if (!ctx) return "";
  gtable_dev& g = g_gtable[ctx->device];
  std::lock_guard<std::mutex> lock(g.m);
  snprintf(ctx->gt_note, sizeof ctx->gt_note, "%s", g.note);
  return ctx->gt_note;
}
// blocks until the background build of the context's device has ended (either way); returns the window bits in use then
int s2k_ctx_gt_wait(s2k_ctx* ctx) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  gtable_dev& g = g_gtable[ctx->device];
  std::unique_lock<std::mutex> lock(g.m);
  g.cv.wait(lock, [&] { return !g.building; });
  return ctx->gt_fixed ? ctx->gt_fixed : g.auto_bits.load();
}
// Test hook (tests/test_gpu_round6.py): the next s2k_ecdsa_verify_batch_device call of this (automatic) context publishes the
// table of `bits` for the device's automatic contexts BETWEEN its ladder launch and its worklist launch - the moment the
// background build must not be visible inside a call.  One shot; 0 disarms.
int s2k_debug_gt_swap_in_call(s2k_ctx* ctx, int bits) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (bits != 0 && (bits < 16 || bits > GT_BITS_MAX)) return fail(ctx, S2K_ERR_ARG, "generator window width %d: 0 or 16 .. %d", bits, GT_BITS_MAX);
  if (ctx->gt_fixed && bits) return fail(ctx, S2K_ERR_ARG, "a context with an explicit table width never changes tables");
  ctx->dbg_gt_swap = bits;
  return S2K_OK;
}
}  // extern "C"
