// keyset.hip — key sets (s2k_keyset_*): the set and its index, growing it, and the verification entry points over it, by key
// index and by key bytes, synchronous and as tickets.  The kernels, their launchers, the context and the ticket plumbing are
// engine.hip's (engine_internal.h); the table builds and the sort keyed.hip's; the index's kernels keyset_index.hip's.  Two small
// kernels live here: k_ks_expand_x (the x-only keys of a BIP-340 call by index) and k_ks_debug_entries (the test hook
// s2k_debug_keyset_entries: a set's tables read back).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>

#include <sys/random.h>

#include "engine_internal.h"
#include "keyset_index.h"
#include "lane_tables.h"

using namespace s2k;

extern "C" {

// ---------------------------------------------------------------------------------------
// Key sets: the per-key tables of a fixed list of public keys, built once and kept (the device analogue of what a
// secec.PublicKey caches per key, secec/secec.go:80-85,188-216: the decoded point and its encoding).  A verification
// call names each signature's key by index; nothing is grouped and no table is built inside the call.
// ---------------------------------------------------------------------------------------
struct s2k_keyset {
  s2k_ctx* ctx;       // the owner (compared, never followed after creation: the set may outlive it by accident)
  uint64_t generation;   // of the owner: a context destroyed and another created at the same address is not the owner
  int device;
  size_t n;           // live keys: what bounds a key index and sizes a call's scratch
  size_t cap;         // keys the buffers have room for (>= n): every offset into `base` and `joint` comes from it
  uint8_t* base;      // device: keys | tables | validity | identity | counters (s2k_internal_keyset_bytes of cap)
  size_t bytes;
  uint4* joint;       // device: the joint tables (320 KiB per key; 0.81 / 2.75 MiB at 5- / 6-bit digits), or null: the ladder over the 32-chunk tables
  size_t joint_bytes;
  int jw;             // digit width of the joint tables: 4, 5 or 6 (0: none)
  int chunks;         // geometry of the tables in `base`: KS_CHUNKS, or KC_TEETH - a comb set (S2K_KEYSET_COMB; never with joint tables)
  // the index, key bytes -> key index (s2k_keyset_index_create; keyset_index.h): an allocation of its own, not counted in `bytes`
  uint64_t* index;    // device: 2^index_log2 slots, then S2K_KSI_INFO_WORDS counters (null: the set has no index)
  uint32_t index_log2;
  uint64_t index_seed;          // hash seed (operating-system randomness, per set)
  uint64_t index_occupied, index_longest;   // distinct 64-byte keys; longest probe distance of a stored entry
};

// The ladder of a key-set call, from the set's layout: the ECDSA mode, or its BIP-340 counterpart (the ECDSA mode + 4; a comb
// set runs the ladder of a call's comb tables over the set's)
static_assert(MODE_SCHNORR_KEYSET == MODE_ECDSA_KEYSET + 4 && MODE_SCHNORR_KEYSET_JOINT == MODE_ECDSA_KEYSET_JOINT + 4 &&
                  MODE_SCHNORR_KEYSET_JOINT5 == MODE_ECDSA_KEYSET_JOINT5 + 4 && MODE_SCHNORR_KEYSET_JOINT6 == MODE_ECDSA_KEYSET_JOINT6 + 4,
              "BIP-340 over a key set: the ECDSA mode + 4");
static int keyset_ladder_mode(const s2k_keyset* ks, bool schnorr) {
  if (ks->chunks == KC_TEETH) return schnorr ? MODE_SCHNORR_COMB : MODE_ECDSA_COMB;
  const int m = !ks->joint ? MODE_ECDSA_KEYSET : ks->jw == 6 ? MODE_ECDSA_KEYSET_JOINT6 : ks->jw == 5 ? MODE_ECDSA_KEYSET_JOINT5 : MODE_ECDSA_KEYSET_JOINT;
  return schnorr ? m + 4 : m;
}

int s2k_keyset_create(s2k_ctx* ctx, size_t n_keys, const uint8_t* pub_xy, s2k_keyset** out) {
  return s2k_keyset_create_cap(ctx, n_keys, pub_xy, S2K_KEYSET_AUTO, 0, out);
}
int s2k_keyset_create_ex(s2k_ctx* ctx, size_t n_keys, const uint8_t* pub_xy, int layout, s2k_keyset** out) {
  return s2k_keyset_create_cap(ctx, n_keys, pub_xy, layout, 0, out);
}
// capacity: keys the set has memory for (0: n_keys).  Every buffer is laid out for it; the tables of n_keys keys are built.
int s2k_keyset_create_cap(s2k_ctx* ctx, size_t n_keys, const uint8_t* pub_xy, int layout, size_t capacity, s2k_keyset** out) {
  if (!ctx || !out) return fail(ctx, S2K_ERR_ARG, "null argument");
  if (layout != S2K_KEYSET_AUTO && layout != S2K_KEYSET_CHUNKS && layout != S2K_KEYSET_JOINT && layout != S2K_KEYSET_JOINT5 &&
      layout != S2K_KEYSET_JOINT6 && layout != S2K_KEYSET_COMB)
    return fail(ctx, S2K_ERR_ARG, "unknown key-set layout");
  *out = nullptr;
  if (n_keys == 0 || !pub_xy) return fail(ctx, S2K_ERR_ARG, "empty key set");
  if (n_keys > 0x0fffffffu) return fail(ctx, S2K_ERR_ARG, "key set too large");
  const size_t cap = capacity ? capacity : n_keys;
  if (cap < n_keys || cap > 0x0fffffffu) return fail(ctx, S2K_ERR_ARG, "key set of %zu keys with a capacity of %zu (n_keys .. 0x0fffffff)", n_keys, cap);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_streams(ctx);
  if (rc) return rc;
  s2k_keyset* ks = new (std::nothrow) s2k_keyset();
  if (!ks) return fail(ctx, S2K_ERR_NOMEM, "out of host memory");
  ks->ctx = ctx;
  ks->generation = ctx->generation;
  ks->device = ctx->device;
  ks->n = n_keys;
  ks->cap = cap;
  size_t off[5];
  ks->chunks = layout == S2K_KEYSET_COMB ? KC_TEETH : KS_CHUNKS;
  ks->bytes = s2k_internal_keyset_bytes(cap, off, ks->chunks);
  hipError_t e = hipMalloc((void**)&ks->base, ks->bytes);
  if (e != hipSuccess) {
    delete ks;
    return fail(ctx, S2K_ERR_HIP, "key set of %zu keys (%zu bytes): %s", cap, ks->bytes, hipGetErrorString(e));
  }
  hipStream_t st = ctx->s_comp;
  rc = ctx_enter(ctx, st);
  if (rc == S2K_OK && hipMemcpyAsync(s2k_internal_keyset_view(ks->base, cap, ks->chunks).keys, pub_xy, n_keys * 64, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = fail(ctx, S2K_ERR_HIP, "copy of the keys failed");
  if (rc == S2K_OK) rc = s2k_internal_keyset_build(ctx, ks->base, cap, 0, n_keys, st, ks->chunks);
  // joint tables (one table addition per digit position instead of two; 320 KiB per key on top, 0.81 MiB at 5-bit digits: 26
  // positions, 2.75 MiB at 6-bit digits: 22): the layout asked for, or - S2K_KEYSET_AUTO - the widest of 5 and 4 bits that takes no
  // more than half of the device memory that is free now (2^16 keys at 5 bits are 56 GB: a quarter would ask for a device with
  // 224 GB free, which the 288 GB one never has once a context lives on it).  The tables are sized, and the layout chosen, by
  // the CAPACITY; the build's scratch by the keys there are
  ks->joint = nullptr;
  ks->joint_bytes = 0;
  ks->jw = 0;
  uint4* scratch = nullptr;
  if (rc == S2K_OK && layout != S2K_KEYSET_CHUNKS && layout != S2K_KEYSET_COMB) {
    int w = layout == S2K_KEYSET_JOINT6 ? 6 : layout == S2K_KEYSET_JOINT5 ? 5 : layout == S2K_KEYSET_JOINT ? 4 : 0;
    // s2k_set_table_memory_budgets: no more than this many bytes count as free for joint tables (an operator's cap - and how
    // the choice of S2K_KEYSET_AUTO and the failure of an explicit layout are exercised without filling a 288 GB device)
    const size_t pretend_free = s2k_internal_keyset_budget() ? s2k_internal_keyset_budget() : ~(size_t)0;
    if (w == 0) {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
        const size_t promised = s2k_internal_gt_pending_bytes(ctx->device);   // what the background table build is about to take
        free_b -= promised < free_b ? promised : free_b;
        if (free_b > pretend_free) free_b = pretend_free;
        if (s2k_internal_keyset_joint_bytes(cap, 5) + s2k_internal_keyset_joint_scratch_bytes(n_keys, 5) <= free_b / 2) w = 5;
        else if (s2k_internal_keyset_joint_bytes(cap, 4) <= free_b / 2) w = 4;
      }
    }
    if (w) {
      const size_t want = s2k_internal_keyset_joint_bytes(cap, w), want_scr = s2k_internal_keyset_joint_scratch_bytes(n_keys, w);
      hipError_t e2 = want + want_scr > pretend_free ? hipErrorOutOfMemory : hipMalloc((void**)&ks->joint, want);
      if (e2 == hipSuccess && want_scr) e2 = hipMalloc((void**)&scratch, want_scr);
      if (e2 == hipSuccess) {
        ks->joint_bytes = want;
        ks->jw = w;
        rc = w == 4 ? s2k_internal_keyset_build_joint(ctx, ks->base, cap, 0, n_keys, ks->joint, st)
                    : s2k_internal_keyset_build_joint_wide(ctx, ks->base, cap, 0, n_keys, w, ks->joint, scratch, st);
      } else {
        (void)hipGetLastError();
        if (ks->joint) (void)hipFree(ks->joint);
        ks->joint = nullptr;
        if (layout != S2K_KEYSET_AUTO) rc = fail(ctx, S2K_ERR_HIP, "joint tables of %zu keys (%zu bytes): %s", cap, want + want_scr, hipGetErrorString(e2));
      }
    }
  }
  if (rc == S2K_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(ctx, S2K_ERR_HIP, "key set build failed");
  if (scratch) {
    (void)hipStreamSynchronize(st);
    (void)hipFree(scratch);
  }
  ctx->have_last = false;
  if (rc) {
    if (ks->joint) (void)hipFree(ks->joint);
    (void)hipFree(ks->base);
    delete ks;
    return rc;
  }
  *out = ks;
  return S2K_OK;
}
void s2k_keyset_destroy(s2k_keyset* ks) {
  if (!ks) return;
  (void)hipSetDevice(ks->device);
  (void)hipDeviceSynchronize();
  if (ks->joint) (void)hipFree(ks->joint);
  if (ks->index) (void)hipFree(ks->index);
  (void)hipFree(ks->base);
  delete ks;
}
size_t s2k_keyset_size(const s2k_keyset* ks) { return ks ? ks->n : 0; }
size_t s2k_keyset_capacity(const s2k_keyset* ks) { return ks ? ks->cap : 0; }
size_t s2k_keyset_device_bytes(const s2k_keyset* ks) { return ks ? ks->bytes + ks->joint_bytes : 0; }
int s2k_keyset_layout(const s2k_keyset* ks) {
  return !ks ? 0 : ks->chunks == KC_TEETH ? S2K_KEYSET_COMB : !ks->joint ? S2K_KEYSET_CHUNKS : ks->jw == 6 ? S2K_KEYSET_JOINT6 : ks->jw == 5 ? S2K_KEYSET_JOINT5 : S2K_KEYSET_JOINT;
}
// pure host function: what a layout costs per signature and per key, from the geometries the kernels are built on
int s2k_keyset_geometry(int layout, uint64_t out[3]) {
  if (!out) return fail(nullptr, S2K_ERR_ARG, "null argument");
  const uint64_t chunk_bytes = (uint64_t)KS_SLOTS * 128;
  switch (layout) {
    case S2K_KEYSET_CHUNKS:
      out[0] = 2 * KS_CHUNKS;
      out[1] = 0;
      out[2] = chunk_bytes;
      return S2K_OK;
    case S2K_KEYSET_JOINT:
      out[0] = KS_CHUNKS;
      out[1] = 0;
      out[2] = chunk_bytes + KJ_KEY_QUADS * sizeof(uint4);
      return S2K_OK;
    case S2K_KEYSET_JOINT5:
      out[0] = kjw_geom<5>::POS;
      out[1] = 0;
      out[2] = chunk_bytes + kjw_geom<5>::KEY_QUADS * sizeof(uint4);
      return S2K_OK;
    case S2K_KEYSET_JOINT6:
      out[0] = kjw_geom<6>::POS;
      out[1] = 0;
      out[2] = chunk_bytes + kjw_geom<6>::KEY_QUADS * sizeof(uint4);
      return S2K_OK;
    case S2K_KEYSET_COMB:
      out[0] = 2 * kc_geom::SPACING;
      out[1] = kc_geom::SPACING - 1;
      out[2] = (uint64_t)KC_SLOTS * 128;
      return S2K_OK;
    default:
      return fail(nullptr, S2K_ERR_ARG, "key-set layout %d has no fixed geometry", layout);
  }
}
int s2k_keyset_valid_keys(s2k_keyset* ks, uint8_t* valid) {
  if (!ks || !valid) return fail(nullptr, S2K_ERR_ARG, "null argument");
  const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
  HIP_TRY(nullptr, hipSetDevice(ks->device));
  HIP_TRY(nullptr, hipMemcpy(valid, v.valid, ks->n, hipMemcpyDeviceToHost));
  return S2K_OK;
}

// ---------------------------------------------------------------------------------------
// Test hook (s2k_debug_keyset_entries): the tables of one key read back entry by entry, through the loaders the ladders read
// them with (ke_load / ke_load3, je_load), reduced and big-endian; a wide joint entry as the eight words per coordinate it
// is stored as.  No kernel of the library is involved: one thread per entry of the range, null stream.
// ---------------------------------------------------------------------------------------
}  // extern "C"
namespace {
enum { KSD_SCALE = 0, KSD_BASE = 1, KSD_JOINT4 = 2, KSD_JOINTW = 3 };
static_assert(kjw_geom<5>::EQ == kjw_geom<6>::EQ, "one entry size for both wide layouts: KSD_JOINTW steps by it whatever the width");
// entries of a section of the set's layout (0: the layout has no such section)
size_t ksd_section_entries(const s2k_keyset* ks, int section) {
  const int jw = ks->joint ? ks->jw : 0;
  if (section == 0) return 1;
  if (section == 1) return ks->chunks == KC_TEETH ? kc_geom::ENTRIES : kt_geom<KS_CHUNKS>::ENTRIES;
  if (section == 2 && jw) return jw == 6 ? kjw_geom<6>::LEAD + 2 : jw == 5 ? kjw_geom<5>::LEAD + 2 : (size_t)KS_CHUNKS * KJ_PER_CHUNK;
  return 0;
}
__device__ __forceinline__ void ksd_store(uint8_t* o, const fe29& v) {
  uint32_t w[8];
  fe29_to_words(w, fe29_normalize(v));
  store_be32_unaligned(o, w);
}
// src: the first entry of the range (KSD_SCALE: the entry that holds W, `elem` its element); out: count * 32 / 96 / 64 / 64 bytes
__global__ void __launch_bounds__(64)
k_ks_debug_entries(int kind, const uint4* __restrict__ src, uint32_t count, int elem, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= count) return;
  if (kind == KSD_SCALE) {
    ksd_store(out, ke_load(src, elem));
  } else if (kind == KSD_BASE) {
    fe29 x, y, bx;
    ke_load3(src + (size_t)i * 8, x, y, bx);
    ksd_store(out + (size_t)i * 96, x);
    ksd_store(out + (size_t)i * 96 + 32, y);
    ksd_store(out + (size_t)i * 96 + 64, bx);
  } else if (kind == KSD_JOINT4) {
    fe29 x, y;
    je_load(src + (size_t)i * KJ_ENTRY_QUADS, x, y);
    ksd_store(out + (size_t)i * 64, x);
    ksd_store(out + (size_t)i * 64 + 32, y);
  } else {
    // (what jw_load cuts into limbs: the words themselves, most significant first - canonical or not is the caller's to see)
    const uint4* e = src + (size_t)i * kjw_geom<5>::EQ;
    const uint4 a = e[0], b = e[1], c = e[2], d = e[3];
    const uint32_t xw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, yw[8] = {c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
    store_be32_unaligned(out + (size_t)i * 64, xw);
    store_be32_unaligned(out + (size_t)i * 64 + 32, yw);
  }
}
}  // namespace
extern "C" {
int s2k_debug_keyset_section_entries(const s2k_keyset* ks, int section, size_t* entries) {
  if (!ks || !entries) return fail(nullptr, S2K_ERR_ARG, "null argument");
  const size_t n = ksd_section_entries(ks, section);
  if (!n) return fail(nullptr, S2K_ERR_ARG, "the layout of the key set has no section %d", section);
  *entries = n;
  return S2K_OK;
}
int s2k_debug_keyset_entries(s2k_keyset* ks, size_t key, int section, size_t first, size_t count, uint8_t* out) {
  if (!ks || !out) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (key >= ks->n) return fail(nullptr, S2K_ERR_ARG, "key %zu of a set of %zu", key, ks->n);
  const bool comb = ks->chunks == KC_TEETH;
  const int jw = ks->joint ? ks->jw : 0;
  const size_t entries = ksd_section_entries(ks, section), out_bytes = section == 0 ? 32 : section == 1 ? 96 : 64;
  if (!entries) return fail(nullptr, S2K_ERR_ARG, "the layout of the key set has no section %d", section);
  if (first > entries || count > entries - first) return fail(nullptr, S2K_ERR_ARG, "entries %zu + %zu of a section of %zu", first, count, entries);
  if (section == 0 && count != 1) return fail(nullptr, S2K_ERR_ARG, "section 0 is one value");
  if (count == 0) return S2K_OK;
  const uint4* kt = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks).tables + key * (size_t)(comb ? KC_SLOTS : KS_SLOTS) * 8;
  using GS = kt_geom<KS_CHUNKS>;
  const uint4* src;
  int kind, elem = 0;
  if (section == 0) {
    kind = KSD_SCALE;
    src = kt + (size_t)(comb ? kc_geom::WENT : GS::SCR + GS::W_SLOT / 3) * 8;
    elem = comb ? kc_geom::W : GS::W_SLOT % 3;
  } else if (section == 1) {
    kind = KSD_BASE;
    src = kt + first * 8;
  } else if (jw == 4) {
    kind = KSD_JOINT4;
    src = ks->joint + key * KJ_KEY_QUADS + first * KJ_ENTRY_QUADS;
  } else {
    kind = KSD_JOINTW;
    src = ks->joint + key * (jw == 6 ? kjw_geom<6>::KEY_QUADS : kjw_geom<5>::KEY_QUADS) + first * kjw_geom<5>::EQ;
  }
  HIP_TRY(nullptr, hipSetDevice(ks->device));
  dev_buf o;
  HIP_TRY(nullptr, o.alloc(count * out_bytes));
  k_ks_debug_entries<<<(unsigned)((count + 63) / 64), 64>>>(kind, src, (uint32_t)count, elem, (uint8_t*)o.p);
  HIP_TRY(nullptr, hipGetLastError());
  HIP_TRY(nullptr, hipDeviceSynchronize());
  HIP_TRY(nullptr, hipMemcpy(out, o.p, count * out_bytes, hipMemcpyDeviceToHost));
  return S2K_OK;
}

// ---------------------------------------------------------------------------------------
// The lane-per-signature path over a set: the steps its four flows share.  A flow is entered (ctx_enter) on the caller's
// stream `st` and reads as the list of its own stages between these steps - its preparation kernel on the second stream, by
// key bytes the lookup in front of the sort, its tail of ladders, finish and worklist kernels, and its stage-timing marks.
// ---------------------------------------------------------------------------------------
// Workspace, second stream, the sort's scratch and the flow's own buffer (*own: xkeys or ks_found; null: none), in this order
// and BEFORE the fork (growing a buffer synchronises the device); then the call's worklist counter and its verdicts zeroed:
// signatures that end on no ladder lane stay invalid
static int ks_lane_begin(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, void* d_valid, hipStream_t st, void** own, size_t* own_bytes,
                         size_t own_need, lane_ws* w) {
  int rc = s2k_internal_ensure_ws(ctx, n);
  if (rc) return rc;
  rc = ctx_aux_streams(ctx);
  if (rc) return rc;
  rc = s2k_internal_keyset_reserve(ctx, ks->n, n);
  if (rc) return rc;
  if (own) rc = ctx_reserve(ctx, own, own_bytes, own_need);
  if (rc) return rc;
  *w = lane_ws_of(ctx, n);
  ctx->ks_last = S2K_KEYSET_LADDER_LANE;
  ctx->last_wl_count = w->wl_count;
  HIP_TRY(ctx, hipMemsetAsync(w->wl_count, 0, sizeof(uint32_t), st));
  HIP_TRY(ctx, hipMemsetAsync(d_valid, 0, n, st));
  return S2K_OK;
}
// the second stream takes up where the caller's stands: the flow's preparation and the generator part go there
static int ks_lane_fork(s2k_ctx* ctx, hipStream_t st) {
  HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->s_aux, ctx->ev_fork, 0));
  return S2K_OK;
}
static int ks_lane_launched(s2k_ctx* ctx) { return hipGetLastError() == hipSuccess ? S2K_OK : fail(ctx, S2K_ERR_HIP, "launch failed"); }
// the set's index asked for n keys on `st` (key_bytes: as s2k_internal_ksi_lookup takes it)
static int keyset_index_lookup(s2k_ctx* ctx, const s2k_keyset* ks, hipStream_t st, size_t n, const uint8_t* d_keys, int key_bytes, size_t stride,
                               uint32_t* d_out) {
  const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
  return s2k_internal_ksi_lookup(ctx, st, v.keys, ks->index, ks->index_log2, ks->index_seed, v.valid, n, d_keys, key_bytes, stride, d_out);
}
// Behind the fork (rc: how the launches on the second stream and, by key bytes, the lookup went): the sort by the key indices
// `kidx` on the caller's stream - an index outside the set, 0xFFFFFFFF of a lookup among them, lands in the list `left` -, the
// join whatever happened, and *kg completed for the set's ladder.  After an error the call is left: nothing of it stays in
// flight on a stream the next call does not wait for
static int ks_lane_sort_join(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* kidx, hipStream_t st, const lane_ws& w, int rc,
                             key_groups* kg) {
  if (rc == S2K_OK) rc = s2k_internal_keyset_sort(ctx, ks->base, ks->cap, ks->n, n, kidx, st, kg, ks->chunks);
  ctx_aux_join(ctx, st);
  if (rc) {
    (void)ctx_leave(ctx, st);
    return rc;
  }
  kg->gp = w.gp;
  kg->jtab = ks->joint;
  return S2K_OK;
}

// s2k_ecdsa_verify_batch_keyset_device above the row threshold.  Stage times (s2k_ctx_profile_read_stages): [0] + [1] the sort
// with the second stream's work beside it, [2] the ladder, [3] the worklist kernel, [4] nothing
static int ecdsa_keyset_lane(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* kidx, const uint8_t* dig, const uint8_t* r,
                             const uint8_t* s, uint32_t flags, uint8_t* valid, hipStream_t st) {
  lane_ws w;
  int rc = ks_lane_begin(ctx, ks, n, valid, st, nullptr, nullptr, 0, &w);
  if (rc) return rc;
  const uint32_t kvf = (flags & S2K_ECDSA_FORCE_WORKLIST) ? KVF_FORCE_WORKLIST : 0u;
  prof_mark(ctx, st, 0);
  prof_mark(ctx, st, 1);
  rc = ks_lane_fork(ctx, st);
  if (rc) return rc;
  launch_scalar_prep(ctx->s_aux, w, 0, n, prep_lanes(n), dig, r, s, nullptr, flags);
  launch_generator_part(ctx, ctx->s_aux, w, 0u, (uint32_t)n);
  key_groups kg{};
  rc = ks_lane_sort_join(ctx, ks, n, kidx, st, w, ks_lane_launched(ctx), &kg);
  if (rc) return rc;
  prof_mark(ctx, st, 2);
  // (the keyed prologue reads no key: pub is null)
  launch_ladder(ctx, st, keyset_ladder_mode(ks, /*schnorr=*/false), n, kvf, nullptr, r, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, kg);
  prof_mark(ctx, st, 3);
  HIP_TRY(ctx, hipGetLastError());
  launch_verify_fallback_keyset(ctx, st, n, w, s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks).keys, kidx, dig, r, s, flags, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

int s2k_ecdsa_verify_batch_keyset_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_key_index, const void* d_dig,
                                         const void* d_r, const void* d_s, uint32_t flags, void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  // (a child context of submit / wait verifies over its parent's key sets: the tables are only read)
  const s2k_ctx* owner = ctx->parent ? ctx->parent : ctx;
  if (!ks || ks->ctx != owner || ks->generation != owner->generation || ks->device != ctx->device)
    return fail(ctx, S2K_ERR_ARG, "key set of another context");
  if (n == 0) return S2K_OK;
  if (!d_key_index || !d_dig || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  if (flags & S2K_ECDSA_FORCE_COMPLETE) return fail(ctx, S2K_ERR_ARG, "S2K_ECDSA_FORCE_COMPLETE does not apply to key sets");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  const bool comb = ks->chunks == KC_TEETH;
  if (n <= (comb ? ctx->ks_comb_row_max : ctx->ks_row_max) && !(flags & (S2K_ECDSA_FORCE_WORKLIST | S2K_ECDSA_FORCE_COMPLETE))) {
    // small calls: a wave per signature over the set's 32-chunk tables (k_verify_row_keyset) or, where the caller asked for it
    // (s2k_ctx_set_keyset_comb_small_batch_max), over a comb set's tables (k_verify_row_comb), one launch; nothing is sorted
    // and nothing is left for a worklist
    const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
    ctx->ks_last = comb ? S2K_KEYSET_LADDER_ROW_COMB : S2K_KEYSET_LADDER_ROW;
    ctx->kg_counters = nullptr;
    ctx->last_wl_count = nullptr;
    prof_mark(ctx, st, 0);
    prof_mark(ctx, st, 1);
    prof_mark(ctx, st, 2);
    (comb ? launch_verify_row_comb : launch_verify_row_keyset)(ctx, st, n, ks->n, (const uint32_t*)d_key_index, v.tables, v.valid,
                                                               (const uint8_t*)d_dig, (const uint8_t*)d_r, (const uint8_t*)d_s, flags, (uint8_t*)d_valid);
    HIP_TRY(ctx, hipGetLastError());
    prof_mark(ctx, st, 3);
    prof_mark(ctx, st, 4);
    prof_mark(ctx, st, 5);
    return ctx_leave(ctx, st);
  }
  return ecdsa_keyset_lane(ctx, ks, n, (const uint32_t*)d_key_index, (const uint8_t*)d_dig, (const uint8_t*)d_r, (const uint8_t*)d_s, flags,
                           (uint8_t*)d_valid, st);
}

int s2k_ecdsa_verify_batch_keyset(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* key_index, const uint8_t* dig,
                                  const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!key_index || !dig || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const stage_part parts[5] = {stage_in(key_index, n * 4), stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 5, n * 100, s2k_internal_small_call(ctx, n, flags), [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_batch_keyset_device(c, ks, n, d[0], d[1], d[2], d[3], flags, d[4], st);
  });
}

// ---------------------------------------------------------------------------------------
// Key sets by key bytes: the index of a set (keyset_index.h / keyset_index.hip) resolves the key bytes a caller has to the
// key indices the set's tables are named by, on the device; s2k_ecdsa_verify_batch_keyset_bykey joins the lookup, the set's
// ladder for the keys it knows and the general ladder for the rest, without a host round trip in between.
// ---------------------------------------------------------------------------------------
int s2k_keyset_index_geometry(size_t n_keys, uint32_t log2_slots, uint64_t out[2]) {
  if (!out) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (!ksi_geometry(n_keys, log2_slots, out))
    return fail(nullptr, S2K_ERR_ARG, "key-set index: %zu keys in 2^%u slots (more slots than keys, at most 2^31; 1 .. 0x0fffffff keys)", n_keys, log2_slots);
  return S2K_OK;
}
// A fresh index of the keys 0 .. nkeys - 1 of the set in 2^lg slots: allocated, filled and read back on the null stream
// (synchronous).  The set is not touched: the caller puts the table in (keyset_index_adopt).
// (its two halves apart for s2k_keyset_replace, which allocates before it writes a row and fills afterwards: keyset_index_alloc,
// and keyset_index_fill, which frees the table when it fails)
static int keyset_index_alloc(uint32_t lg, uint64_t** out_slots) {
  const size_t bytes = ((size_t)1 << lg) * sizeof(uint64_t);
  hipError_t e = hipMalloc((void**)out_slots, bytes + S2K_KSI_INFO_WORDS * sizeof(uint32_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *out_slots = nullptr;
    return fail(nullptr, S2K_ERR_NOMEM, "key-set index of %zu bytes: %s", bytes, hipGetErrorString(e));
  }
  return S2K_OK;
}
static int keyset_index_fill(const s2k_keyset* ks, size_t nkeys, uint32_t lg, uint64_t seed, uint64_t* slots, uint32_t h[S2K_KSI_INFO_WORDS]) {
  const size_t nslots = (size_t)1 << lg, bytes = nslots * sizeof(uint64_t);
  uint32_t* info = reinterpret_cast<uint32_t*>(slots + nslots);
  const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
  int rc = S2K_OK;
  if (hipMemsetAsync(slots, 0xff, bytes, nullptr) != hipSuccess || hipMemsetAsync(info, 0, S2K_KSI_INFO_WORDS * sizeof(uint32_t), nullptr) != hipSuccess)
    rc = fail(nullptr, S2K_ERR_HIP, "key-set index: memset failed");
  if (rc == S2K_OK) rc = s2k_internal_ksi_build(nullptr, nullptr, v.keys, 0, nkeys, slots, lg, seed, info);
  if (rc == S2K_OK && hipMemcpy(h, info, S2K_KSI_INFO_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
    rc = fail(nullptr, S2K_ERR_HIP, "key-set index build failed");
  // (cannot happen while there are more slots than keys: every probe loop is bounded all the same, and says so here)
  if (rc == S2K_OK && h[S2K_KSI_FAILED]) rc = fail(nullptr, S2K_ERR_HIP, "key-set index: an insert found no slot");
  if (rc) {
    (void)hipDeviceSynchronize();
    (void)hipFree(slots);
  }
  return rc;
}
static int keyset_index_make(const s2k_keyset* ks, size_t nkeys, uint32_t lg, uint64_t seed, uint64_t** out_slots, uint32_t h[S2K_KSI_INFO_WORDS]) {
  uint64_t* slots = nullptr;
  int rc = keyset_index_alloc(lg, &slots);
  if (rc == S2K_OK) rc = keyset_index_fill(ks, nkeys, lg, seed, slots, h);
  if (rc) return rc;
  *out_slots = slots;
  return S2K_OK;
}
// (no call that uses the set is in progress and the device is idle: the table it had, if any, is freed)
static void keyset_index_adopt(s2k_keyset* ks, uint64_t* slots, uint32_t lg, uint64_t seed, const uint32_t h[S2K_KSI_INFO_WORDS]) {
  if (ks->index) (void)hipFree(ks->index);
  ks->index = slots;
  ks->index_log2 = lg;
  ks->index_seed = seed;
  ks->index_occupied = h[S2K_KSI_OCCUPIED];
  ks->index_longest = h[S2K_KSI_LONGEST];
}
static uint32_t keyset_index_auto_log2(size_t n_keys) {
  uint64_t geo[2] = {0, 0};
  (void)ksi_geometry(n_keys, 0, geo);
  uint32_t lg = 0;
  while (((uint64_t)1 << lg) < geo[0]) ++lg;
  return lg;
}
// The index of the keys 0 .. nkeys - 1 anew, at the automatic geometry of the set's capacity and with the seed it has
static int keyset_index_rebuild(s2k_keyset* ks, size_t nkeys) {
  const uint32_t lg = keyset_index_auto_log2(ks->cap);
  uint64_t* slots = nullptr;
  uint32_t h[S2K_KSI_INFO_WORDS] = {0, 0, 0, 0};
  const int rc = keyset_index_make(ks, nkeys, lg, ks->index_seed, &slots, h);
  if (rc) return rc;
  keyset_index_adopt(ks, slots, lg, ks->index_seed, h);
  return S2K_OK;
}
int s2k_keyset_index_create(s2k_keyset* ks, uint32_t log2_slots) {
  if (!ks) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (ks->index) return fail(nullptr, S2K_ERR_ARG, "the key set has an index already");
  // 0: sized for the capacity, so that appends up to it never rebuild (cap == n: what it always was); an explicit size is
  // the caller's, and only has to hold the keys there are
  uint64_t geo[2];
  if (!ksi_geometry(log2_slots ? ks->n : ks->cap, log2_slots, geo))
    return fail(nullptr, S2K_ERR_ARG, "key-set index: %zu keys in 2^%u slots (more slots than keys, at most 2^31)", ks->n, log2_slots);
  uint32_t lg = 0;
  while (((uint64_t)1 << lg) < geo[0]) ++lg;
  uint64_t seed = 0;
  if (getrandom(&seed, sizeof seed, 0) != (ssize_t)sizeof seed) seed = 0x5ec9u;
  HIP_TRY(nullptr, hipSetDevice(ks->device));
  HIP_TRY(nullptr, hipDeviceSynchronize());            // (the rule of s2k_keyset_destroy: no call that uses the set is in progress)
  uint64_t* slots = nullptr;
  uint32_t h[S2K_KSI_INFO_WORDS] = {0, 0, 0, 0};
  const int rc = keyset_index_make(ks, ks->n, lg, seed, &slots, h);
  if (rc) return rc;
  keyset_index_adopt(ks, slots, lg, seed, h);
  return S2K_OK;
}

// ---------------------------------------------------------------------------------------
// Growing a set.  The buffers of a set are laid out for its capacity (s2k_keyset_create_cap, s2k_keyset_reserve); an append
// copies the new keys behind the live ones and runs the SAME table kernels as the creation over the new rows only
// (s2k_internal_keyset_build with first > 0), then inserts the new range into the index, and only then moves n: until that
// moment every call sees the old set, and a failure leaves it.  Nothing here goes through a context - as
// s2k_keyset_index_create, on the null stream with the device idle before and after.
// ---------------------------------------------------------------------------------------
// the index after keys first .. first + count - 1 have been written behind the `first` live ones
static int keyset_index_grow(s2k_keyset* ks, size_t first, size_t count) {
  if (first + count >= ((uint64_t)1 << ks->index_log2)) return keyset_index_rebuild(ks, first + count);   // (an explicit geometry, outgrown)
  const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
  uint32_t* info = reinterpret_cast<uint32_t*>(ks->index + ((size_t)1 << ks->index_log2));
  uint32_t h[S2K_KSI_INFO_WORDS] = {0, 0, 0, 0};
  int rc = s2k_internal_ksi_build(nullptr, nullptr, v.keys, first, count, ks->index, ks->index_log2, ks->index_seed, info);
  if (rc) return rc;                // (refused before the launch: the table is as it was)
  if (hipMemcpy(h, info, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(nullptr, S2K_ERR_HIP, "key-set index: inserting the appended keys failed");
  if (rc == S2K_OK && h[S2K_KSI_FAILED]) rc = fail(nullptr, S2K_ERR_HIP, "key-set index: an insert found no slot");
  if (rc == S2K_OK) {
    ks->index_occupied = h[S2K_KSI_OCCUPIED];
    ks->index_longest = h[S2K_KSI_LONGEST];
    return S2K_OK;
  }
  // some slots may name rows that are not going to be keys: the index of the live keys anew - or, failing that too, none
  (void)hipGetLastError();
  const uint32_t lg = ks->index_log2;
  uint64_t* slots = nullptr;
  if (keyset_index_make(ks, first, lg, ks->index_seed, &slots, h) == S2K_OK) keyset_index_adopt(ks, slots, lg, ks->index_seed, h);
  else {
    (void)hipFree(ks->index);
    ks->index = nullptr;
  }
  return rc;
}
static int keyset_append(s2k_keyset* ks, size_t n_new, const void* src, bool on_device, uint32_t* first_index) {
  if (!ks) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (n_new == 0) {
    if (first_index) *first_index = (uint32_t)ks->n;
    return S2K_OK;
  }
  if (!src) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (n_new > ks->cap - ks->n)
    return fail(nullptr, S2K_ERR_ARG, "a key set of %zu keys with a capacity of %zu has no room for %zu more (s2k_keyset_reserve)", ks->n, ks->cap, n_new);
  HIP_TRY(nullptr, hipSetDevice(ks->device));
  HIP_TRY(nullptr, hipDeviceSynchronize());            // (the rule of s2k_keyset_destroy: no call that uses the set is in progress)
  const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
  const size_t first = ks->n;
  uint4* scratch = nullptr;
  const size_t want_scr = ks->joint ? s2k_internal_keyset_joint_scratch_bytes(n_new, ks->jw) : 0;
  if (want_scr && hipMalloc((void**)&scratch, want_scr) != hipSuccess) {
    (void)hipGetLastError();
    return fail(nullptr, S2K_ERR_NOMEM, "key-set append: %zu bytes of build scratch", want_scr);
  }
  int rc = S2K_OK;
  if (hipMemcpy(v.keys + first * 64, src, n_new * 64, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) != hipSuccess)
    rc = fail(nullptr, S2K_ERR_HIP, "copy of the keys failed");
  if (rc == S2K_OK) rc = s2k_internal_keyset_build(nullptr, ks->base, ks->cap, first, n_new, nullptr, ks->chunks);
  if (rc == S2K_OK && ks->joint)
    rc = ks->jw == 4 ? s2k_internal_keyset_build_joint(nullptr, ks->base, ks->cap, first, n_new, ks->joint, nullptr)
                     : s2k_internal_keyset_build_joint_wide(nullptr, ks->base, ks->cap, first, n_new, ks->jw, ks->joint, scratch, nullptr);
  if (rc == S2K_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(nullptr, S2K_ERR_HIP, "key-set append: the table build failed");
  if (scratch) {
    (void)hipDeviceSynchronize();
    (void)hipFree(scratch);
  }
  if (rc == S2K_OK && ks->index) rc = keyset_index_grow(ks, first, n_new);
  if (rc) {
    (void)hipGetLastError();
    (void)hipMemset(v.valid + first, 0, n_new);     // rows past n are "no key"
    return rc;
  }
  ks->n = first + n_new;
  if (first_index) *first_index = (uint32_t)first;
  return S2K_OK;
}
int s2k_keyset_append(s2k_keyset* ks, size_t n_new, const uint8_t* pub_xy, uint32_t* first_index) {
  return keyset_append(ks, n_new, pub_xy, false, first_index);
}
int s2k_keyset_append_device(s2k_keyset* ks, size_t n_new, const void* d_pub_xy, uint32_t* first_index) {
  return keyset_append(ks, n_new, d_pub_xy, true, first_index);
}
// Memory for `capacity` keys: new buffers, the live rows of every section copied to their new offsets, the old buffers freed
// once the copies are done.  Both copies exist for a moment - a set that fills more than half of the device cannot grow this
// way and has to be given its capacity at creation.
int s2k_keyset_reserve(s2k_keyset* ks, size_t capacity) {
  if (!ks) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (capacity <= ks->cap) return S2K_OK;
  if (capacity > 0x0fffffffu) return fail(nullptr, S2K_ERR_ARG, "key set too large");
  HIP_TRY(nullptr, hipSetDevice(ks->device));
  HIP_TRY(nullptr, hipDeviceSynchronize());            // (the rule of s2k_keyset_destroy: no call that uses the set is in progress)
  size_t noff[5];
  const size_t nbytes = s2k_internal_keyset_bytes(capacity, noff, ks->chunks);
  const size_t njoint = ks->joint ? s2k_internal_keyset_joint_bytes(capacity, ks->jw) : 0;
  uint8_t* nbase = nullptr;
  uint4* nj = nullptr;
  hipError_t e = hipMalloc((void**)&nbase, nbytes);
  if (e == hipSuccess && njoint) e = hipMalloc((void**)&nj, njoint);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    if (nbase) (void)hipFree(nbase);
    return fail(nullptr, S2K_ERR_NOMEM, "key set of %zu keys (%zu bytes): %s", capacity, nbytes + njoint, hipGetErrorString(e));
  }
  const size_t n = ks->n, slot_bytes = (size_t)(ks->chunks == KC_TEETH ? KC_SLOTS : KS_SLOTS) * 128;
  const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks), nv = s2k_internal_keyset_view(nbase, capacity, ks->chunks);
  bool ok = hipMemsetAsync(nv.valid, 0, (size_t)((uint8_t*)nv.rep - nv.valid), nullptr) == hipSuccess;     // validity: rows past n are "no key"
  ok = ok && hipMemcpyAsync(nv.keys, v.keys, n * 64, hipMemcpyDeviceToDevice, nullptr) == hipSuccess;
  ok = ok && hipMemcpyAsync(nv.tables, v.tables, n * slot_bytes, hipMemcpyDeviceToDevice, nullptr) == hipSuccess;
  ok = ok && hipMemcpyAsync(nv.valid, v.valid, n, hipMemcpyDeviceToDevice, nullptr) == hipSuccess;
  ok = ok && s2k_internal_keyset_identity(nullptr, nbase, capacity, nullptr, ks->chunks) == S2K_OK;   // the identity of the whole capacity (the counters are the builds' scratch)
  if (ok && nj) ok = hipMemcpyAsync(nj, ks->joint, s2k_internal_keyset_joint_bytes(n, ks->jw), hipMemcpyDeviceToDevice, nullptr) == hipSuccess;
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    (void)hipDeviceSynchronize();
    if (nj) (void)hipFree(nj);
    (void)hipFree(nbase);
    return fail(nullptr, S2K_ERR_HIP, "key-set reserve: copying the set failed");
  }
  if (ks->joint) (void)hipFree(ks->joint);
  (void)hipFree(ks->base);
  ks->base = nbase;
  ks->bytes = nbytes;
  ks->joint = nj;
  ks->joint_bytes = njoint;
  ks->cap = capacity;
  // the index holds key indices, not addresses: it stands - unless it is too small for what the set may now grow to
  if (ks->index && ((uint64_t)1 << ks->index_log2) < 2 * (uint64_t)capacity) return keyset_index_rebuild(ks, ks->n);
  return S2K_OK;
}
// ---------------------------------------------------------------------------------------
// Replacing keys.  The table kernels build table t at row t of a contiguous range, so the new keys' tables are built in a
// STAGING SET - buffers laid out as a set of `piece` keys is, built as a creation of that many keys is - and
// k_ks_scatter_rows (keyset_replace.hip) moves its rows to their slots; a call with more slots than a piece runs piece after
// piece through the same buffers, the (slot, key) pairs in ascending order of the slot.  The launches follow the pieces, never
// the slots.  The index is not patched - a slot of its table belongs to one 64-byte string forever (keyset_index.h) - but
// built anew over the rows 0 .. n - 1, at the geometry and the seed it has, into a table allocated, like everything else the
// call needs, before the first byte of the set changes.  As the append: the null stream, the device idle before and after.
// ---------------------------------------------------------------------------------------
// (src: m keys in the order of `slots`, host or device memory; null: 64 zero bytes each - no point of the curve)
static int keyset_replace(s2k_keyset* ks, size_t m, const uint32_t* slots, const void* src, bool on_device, bool remove) {
  if (!ks) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (m == 0) return S2K_OK;
  if (!slots || (!src && !remove)) return fail(nullptr, S2K_ERR_ARG, "null argument");
  uint32_t* order = new (std::nothrow) uint32_t[m];
  uint32_t* sorted = new (std::nothrow) uint32_t[m];
  uint8_t* keys = (uint8_t*)calloc(m, 64);
  uint8_t *stage = nullptr, *d_slots = nullptr;
  uint4 *stage_joint = nullptr, *scratch = nullptr;
  uint64_t* table = nullptr;
  auto done = [&](int rc) {
    (void)hipFree(stage);
    (void)hipFree(stage_joint);
    (void)hipFree(scratch);
    (void)hipFree(d_slots);
    (void)hipFree(table);
    free(keys);
    delete[] sorted;
    delete[] order;
    return rc;
  };
  if (!order || !sorted || !keys) return done(fail(nullptr, S2K_ERR_NOMEM, "out of host memory"));
  int rc = s2k_internal_keyset_replace_plan(ks->n, m, slots, 0, order, nullptr);
  if (rc) return done(rc);
  size_t piece = s2k_internal_keyset_replace_piece(ks->chunks, ks->joint ? ks->jw : 0);
  if (piece > m) piece = m;
  if (hipSetDevice(ks->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess)      // (the rule of s2k_keyset_destroy: no call that uses the set is in progress)
    return done(fail(nullptr, S2K_ERR_HIP, "key-set replace: the device of the set"));
  if (src && on_device) {
    // (sorted on the host like a caller's host keys: m * 64 bytes come back once)
    uint8_t* given = (uint8_t*)malloc(m * 64);
    if (!given) return done(fail(nullptr, S2K_ERR_NOMEM, "out of host memory"));
    const hipError_t e = hipMemcpy(given, src, m * 64, hipMemcpyDeviceToHost);
    for (size_t j = 0; j < m && e == hipSuccess; ++j) memcpy(keys + j * 64, given + (size_t)order[j] * 64, 64);
    free(given);
    if (e != hipSuccess) return done(fail(nullptr, S2K_ERR_HIP, "copy of the keys failed"));
  } else if (src) {
    for (size_t j = 0; j < m; ++j) memcpy(keys + j * 64, (const uint8_t*)src + (size_t)order[j] * 64, 64);
  }
  for (size_t j = 0; j < m; ++j) sorted[j] = slots[order[j]];
  // everything the call allocates, before the first byte of the set changes
  size_t off[5];
  const size_t stage_bytes = s2k_internal_keyset_bytes(piece, off, ks->chunks);
  const size_t joint_bytes = ks->joint ? s2k_internal_keyset_joint_bytes(piece, ks->jw) : 0;
  const size_t scratch_bytes = ks->joint ? s2k_internal_keyset_joint_scratch_bytes(piece, ks->jw) : 0;
  hipError_t e = hipMalloc((void**)&stage, stage_bytes);
  if (e == hipSuccess && joint_bytes) e = hipMalloc((void**)&stage_joint, joint_bytes);
  if (e == hipSuccess && scratch_bytes) e = hipMalloc((void**)&scratch, scratch_bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d_slots, m * sizeof(uint32_t));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return done(fail(nullptr, S2K_ERR_NOMEM, "key-set replace: %zu bytes of staging for %zu keys a piece: %s", stage_bytes + joint_bytes + scratch_bytes,
                     piece, hipGetErrorString(e)));
  }
  if (ks->index && (rc = keyset_index_alloc(ks->index_log2, &table)) != S2K_OK) return done(rc);
  if (hipMemcpy(d_slots, sorted, m * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
    return done(fail(nullptr, S2K_ERR_HIP, "copy of the slots failed"));
  const keyset_view sv = s2k_internal_keyset_view(stage, piece, ks->chunks);
  bool touched = false;
  for (size_t first = 0; first < m && rc == S2K_OK; first += piece) {
    const size_t count = m - first < piece ? m - first : piece;
    if (hipMemcpy(sv.keys, keys + first * 64, count * 64, hipMemcpyHostToDevice) != hipSuccess) rc = fail(nullptr, S2K_ERR_HIP, "copy of the keys failed");
    if (rc == S2K_OK) rc = s2k_internal_keyset_build(nullptr, stage, piece, 0, count, nullptr, ks->chunks);
    if (rc == S2K_OK && ks->joint)
      rc = ks->jw == 4 ? s2k_internal_keyset_build_joint(nullptr, stage, piece, 0, count, stage_joint, nullptr)
                       : s2k_internal_keyset_build_joint_wide(nullptr, stage, piece, 0, count, ks->jw, stage_joint, scratch, nullptr);
    // (a build that failed has written staging only: the set is as it was)
    if (rc == S2K_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(nullptr, S2K_ERR_HIP, "key-set replace: the table build failed");
    if (rc) break;
    touched = true;
    rc = s2k_internal_keyset_scatter_rows(stage, piece, stage_joint, ks->base, ks->cap, ks->joint, ks->jw, ks->chunks, (const uint32_t*)d_slots + first, count);
    if (rc == S2K_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(nullptr, S2K_ERR_HIP, "key-set replace: moving the rows failed");
  }
  // the index of the rows as they are now - also after a failure that left some of them written - or, failing that, none
  if (ks->index && touched) {
    (void)hipGetLastError();
    uint32_t h[S2K_KSI_INFO_WORDS] = {0, 0, 0, 0};
    const int irc = keyset_index_fill(ks, ks->n, ks->index_log2, ks->index_seed, table, h);
    if (irc == S2K_OK) keyset_index_adopt(ks, table, ks->index_log2, ks->index_seed, h);
    else {
      (void)hipFree(ks->index);
      ks->index = nullptr;
      if (rc == S2K_OK) rc = irc;
    }
    table = nullptr;      // (adopted, or freed by the fill that failed)
  }
  return done(rc);
}
int s2k_keyset_replace(s2k_keyset* ks, size_t m, const uint32_t* slots, const uint8_t* pub_xy) {
  return keyset_replace(ks, m, slots, pub_xy, false, false);
}
int s2k_keyset_replace_device(s2k_keyset* ks, size_t m, const uint32_t* slots, const void* d_pub_xy) {
  return keyset_replace(ks, m, slots, d_pub_xy, true, false);
}
int s2k_keyset_remove(s2k_keyset* ks, size_t m, const uint32_t* slots) { return keyset_replace(ks, m, slots, nullptr, false, true); }
int s2k_keyset_index_info(const s2k_keyset* ks, uint64_t out[4]) {
  if (!ks || !out) return fail(nullptr, S2K_ERR_ARG, "null argument");
  out[0] = ks->index ? (uint64_t)1 << ks->index_log2 : 0;
  out[1] = out[0] * sizeof(uint64_t);
  out[2] = ks->index ? ks->index_occupied : 0;
  out[3] = ks->index ? ks->index_longest : 0;
  return S2K_OK;
}

// what every call by key bytes asks of its set (as the key-set calls do; a child context of submit / wait uses its parent's sets)
static int keyset_index_check(s2k_ctx* ctx, const s2k_keyset* ks) {
  const s2k_ctx* owner = ctx->parent ? ctx->parent : ctx;
  if (!ks || ks->ctx != owner || ks->generation != owner->generation || ks->device != ctx->device)
    return fail(ctx, S2K_ERR_ARG, "key set of another context");
  if (!ks->index) return fail(ctx, S2K_ERR_ARG, "the key set has no index (s2k_keyset_index_create)");
  return S2K_OK;
}

int s2k_keyset_lookup_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_keys, size_t key_bytes, size_t stride,
                             void* d_key_index, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = keyset_index_check(ctx, ks);
  if (rc) return rc;
  if ((key_bytes != 64 && key_bytes != 32 && key_bytes != 33) || stride < key_bytes)
    return fail(ctx, S2K_ERR_ARG, "keys of 64, 32 or 33 bytes, stride >= key_bytes");
  if (n == 0) return S2K_OK;
  if (!d_keys || !d_key_index) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  rc = keyset_index_lookup(ctx, ks, st, n, (const uint8_t*)d_keys, (int)key_bytes, stride, (uint32_t*)d_key_index);
  if (rc) return rc;
  return ctx_leave(ctx, st);
}
int s2k_keyset_lookup(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint8_t* keys, size_t key_bytes, size_t stride,
                      uint32_t* key_index) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = keyset_index_check(ctx, ks);
  if (rc) return rc;
  if ((key_bytes != 64 && key_bytes != 32 && key_bytes != 33) || stride < key_bytes)
    return fail(ctx, S2K_ERR_ARG, "keys of 64, 32 or 33 bytes, stride >= key_bytes");
  if (n == 0) return S2K_OK;
  if (!keys || !key_index) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  const size_t in_bytes = (n - 1) * stride + key_bytes;       // (the last record may end with its key)
  const stage_part parts[2] = {stage_in(keys, in_bytes), stage_out(key_index, n * 4)};
  return s2k_internal_staged_call(ctx, parts, 2, 0, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_keyset_lookup_device(c, ks, n, d[0], key_bytes, stride, d[1], st);
  });
}

// the plain call would take its wave-per-signature or four-lanes-per-signature ladder for this n (verify_batch_device): the
// call by key bytes IS the plain call then, and the set is not used
static bool bykey_delegates(const s2k_ctx* ctx, size_t n, uint32_t flags) {
  const bool ladders = ctx->kg_mode == S2K_KEYS_ADAPTIVE || ctx->kg_mode == S2K_KEYS_OFF;
  return ladders && !(flags & S2K_ECDSA_FORCE_WORKLIST) && (n <= ctx->row_max || n <= ctx->quad_max);
}
static int bykey_check(s2k_ctx* ctx, const s2k_keyset* ks, uint32_t flags) {
  int rc = keyset_index_check(ctx, ks);
  if (rc) return rc;
  if (flags & S2K_ECDSA_FORCE_COMPLETE) return fail(ctx, S2K_ERR_ARG, "S2K_ECDSA_FORCE_COMPLETE does not apply to key sets");
  return S2K_OK;
}
}  // extern "C"
// (for the encoded entry points, ingest.hip: engine_internal.h)
__attribute__((visibility("hidden"))) bool s2k_internal_bykey_delegates(const s2k_ctx* ctx, size_t n, uint32_t flags) {
  return bykey_delegates(ctx, n, flags);
}
__attribute__((visibility("hidden"))) int s2k_internal_bykey_view(s2k_ctx* ctx, const s2k_keyset* ks, uint32_t flags, s2k_bykey_view* out) {
  int rc = bykey_check(ctx, ks, flags);
  if (rc) return rc;
  *out = {s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks), ks->index, ks->index_log2, ks->index_seed};
  return S2K_OK;
}
extern "C" {

int s2k_ecdsa_verify_batch_keyset_bykey_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_pub_xy, const void* d_dig,
                                               const void* d_r, const void* d_s, uint32_t flags, void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = bykey_check(ctx, ks, flags);
  if (rc) return rc;
  if (n == 0) return S2K_OK;
  if (!d_pub_xy || !d_dig || !d_r || !d_s || !d_valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  if (bykey_delegates(ctx, n, flags)) return s2k_ecdsa_verify_batch_device(ctx, n, d_pub_xy, d_dig, d_r, d_s, flags, d_valid, hip_stream);
  return s2k_internal_bykey_device(ctx, ks, n, d_pub_xy, d_dig, d_r, d_s, flags, d_valid, (hipStream_t)hip_stream, nullptr);
}
}  // extern "C"
__attribute__((visibility("hidden"))) int s2k_internal_bykey_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_pub_xy,
                                                                    const void* d_dig, const void* d_r, const void* d_s, uint32_t flags,
                                                                    void* d_valid, hipStream_t st, const uint32_t* d_found) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  const uint8_t *pub = (const uint8_t*)d_pub_xy, *dig = (const uint8_t*)d_dig, *r = (const uint8_t*)d_r, *s = (const uint8_t*)d_s;
  uint8_t* valid = (uint8_t*)d_valid;
  // (a caller that resolved the keys itself did so into the context's buffer, reserved for at least n: it does not move below)
  const size_t found_bytes = ((n + 63) & ~(size_t)63) * sizeof(uint32_t);
  if (d_found && (d_found != ctx->ks_found || ctx->ks_found_bytes < found_bytes))
    return fail(ctx, S2K_ERR_ARG, "key indices outside the context's buffer");
  lane_ws w;
  rc = ks_lane_begin(ctx, ks, n, valid, st, &ctx->ks_found, &ctx->ks_found_bytes, found_bytes, &w);
  if (rc) return rc;
  uint32_t* found = (uint32_t*)ctx->ks_found;
  ctx->kt_last = -1;
  const uint32_t kvf = (flags & S2K_ECDSA_FORCE_WORKLIST) ? KVF_FORCE_WORKLIST : 0u;
  // second stream: scalar preparation and generator part of every signature; caller's: the lookup of the keys, then the sort
  // by the indices it found - a key the set does not hold (0xFFFFFFFF) lands in the list `left`, as an index outside the set does
  prof_mark(ctx, st, 0);
  prof_mark(ctx, st, 1);
  rc = ks_lane_fork(ctx, st);
  if (rc) return rc;
  launch_scalar_prep(ctx->s_aux, w, 0, n, prep_lanes(n), dig, r, s, nullptr, flags);
  launch_generator_part(ctx, ctx->s_aux, w, 0u, (uint32_t)n);
  rc = ks_lane_launched(ctx);
  if (rc == S2K_OK && !d_found) rc = keyset_index_lookup(ctx, ks, st, n, pub, 64, 64, found);
  key_groups kg{};
  rc = ks_lane_sort_join(ctx, ks, n, found, st, w, rc, &kg);
  if (rc) return rc;
  prof_mark(ctx, st, 2);
  // the set's ladder over the keys it holds (its prologue reads no key), the general ladder over the rest with the caller's
  // key bytes, and the complete formulas for the lanes either one tagged: hits and misses alike have their key in d_pub_xy
  launch_ladder(ctx, st, keyset_ladder_mode(ks, /*schnorr=*/false), n, kvf, nullptr, r, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, kg);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 3);
  launch_ladder(ctx, st, MODE_ECDSA_LEFT, n, kvf, pub, r, w, valid, nullptr, nullptr, kg);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  launch_verify_fallback(ctx, st, n, w, pub, dig, r, s, flags, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}
extern "C" {

int s2k_ecdsa_verify_batch_keyset_bykey(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint8_t* pub, const uint8_t* dig,
                                        const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = bykey_check(ctx, ks, flags);
  if (rc) return rc;
  if (n == 0) return S2K_OK;
  if (!pub || !dig || !r || !s || !valid) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (bykey_delegates(ctx, n, flags)) return s2k_ecdsa_verify_batch(ctx, n, pub, dig, r, s, flags, valid);   // (with its small-call route)
  const stage_part parts[5] = {stage_in(pub, n * 64), stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 5, n * 160, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_batch_keyset_bykey_device(c, ks, n, d[0], d[1], d[2], d[3], flags, d[4], st);
  });
}

// ---------------------------------------------------------------------------------------
// BIP-340 over a key set: SchnorrPublicKey.Verify (secec/bitcoin/schnorr.go:221-253) for signatures that name their key by its
// index in a key set.  The set holds X || Y keys; BIP-340's key is the x coordinate and its point lift_x(x), the one with
// even y (NewSchnorrPublicKeyFromPoint, schnorr.go:276-300, does the same to a point): the challenge hashes X, and the
// ladder takes the set's tables with both half scalars' signs flipped where the stored Y is odd.  Same verdicts as
// s2k_schnorr_verify_batch on the expanded x-only key array; what is saved is grouping, key lifts and table build of every
// call, and with joint tables half (or more) of the ladder.
// ---------------------------------------------------------------------------------------
}  // extern "C"
namespace {
// pk32[i] = X of key kidx[i] (zeros for an index outside the set: that signature is on no ladder lane and stays invalid)
__global__ void __launch_bounds__(256)
k_ks_expand_x(uint32_t n, uint32_t nkeys, const uint32_t* __restrict__ kidx, const uint8_t* __restrict__ keys, uint8_t* __restrict__ pk32) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;          // one 16-byte half of a key per thread
  const uint32_t i = t >> 1, h = t & 1u;
  if (i >= n) return;
  const uint32_t k = kidx[i];
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (k < nkeys) v = reinterpret_cast<const uint4*>(keys + (size_t)k * 64)[h];
  reinterpret_cast<uint4*>(pk32 + (size_t)i * 32)[h] = v;
}
}  // namespace
// s2k_schnorr_verify_batch_keyset_device above the row threshold.  No stage times are recorded (and no clock stamps taken)
static int schnorr_keyset_lane(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* kidx, const uint8_t* msgs, const uint64_t* offs,
                               uint32_t mlen, const uint8_t* sig, uint8_t* valid, hipStream_t st) {
  // the expanded x-only keys (what the preparation hashes and the worklist kernel lifts): the context's key-expansion buffer
  lane_ws w;
  int rc = ks_lane_begin(ctx, ks, n, valid, st, &ctx->xkeys, &ctx->xkeys_bytes, n * 32 + 256, &w);
  if (rc) return rc;
  ctx->kg_counters = nullptr;
  uint8_t* pk = (uint8_t*)ctx->xkeys;
  const uint8_t* set_keys = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks).keys;
  k_ks_expand_x<<<blocks_for(2 * n), 256, 0, st>>>((uint32_t)n, (uint32_t)ks->n, kidx, set_keys, pk);
  HIP_TRY(ctx, hipGetLastError());
  // second stream: challenge hashes, scalars and the generator part s*G; caller's: the sort by key index
  rc = ks_lane_fork(ctx, st);
  if (rc) return rc;
  launch_schnorr_prep(ctx->s_aux, n, w, pk, sig, msgs, offs, mlen);
  launch_generator_part(ctx, ctx->s_aux, w, 0u, (uint32_t)n);
  key_groups kg{};
  rc = ks_lane_sort_join(ctx, ks, n, kidx, st, w, ks_lane_launched(ctx), &kg);
  if (rc) return rc;
  // (a comb set: kg.key_bytes == 64 tells MODE_SCHNORR_COMB to flip the signs under an odd Y)
  launch_ladder(ctx, st, keyset_ladder_mode(ks, /*schnorr=*/true), n, 0u, set_keys, sig, w, valid, nullptr, nullptr, kg);
  HIP_TRY(ctx, hipGetLastError());
  launch_affine_finish(st, MODE_SCHNORR, n, (uint32_t)((n + FIN_M - 1) / FIN_M), sig, w, valid, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  // (the worklist kernel re-does its lanes from the x-only key: lift_x gives the even-y point whatever the set's Y says)
  launch_schnorr_worklist(ctx, st, n, w, pk, sig, msgs, offs, mlen, valid);
  HIP_TRY(ctx, hipGetLastError());
  return ctx_leave(ctx, st);
}
extern "C" {
int s2k_schnorr_verify_batch_keyset_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_key_index, const void* d_msgs,
                                           const void* d_msg_offsets, size_t msg_len, const void* d_sig, uint32_t flags, void* d_valid,
                                           void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  const s2k_ctx* owner = ctx->parent ? ctx->parent : ctx;
  if (!ks || ks->ctx != owner || ks->generation != owner->generation || ks->device != ctx->device)
    return fail(ctx, S2K_ERR_ARG, "key set of another context");
  if (n == 0) return S2K_OK;
  if (!d_key_index || !d_sig || !d_valid || (!d_msgs && (d_msg_offsets || msg_len))) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  if (flags) return fail(ctx, S2K_ERR_ARG, "s2k_schnorr_verify_batch_keyset takes no flags");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = ctx_enter(ctx, st);
  if (rc) return rc;
  const bool comb = ks->chunks == KC_TEETH;
  if (n <= (comb ? ctx->ks_comb_row_max : ctx->ks_row_max)) {
    // small calls: a wave per signature over the set's 32-chunk tables (k_schnorr_row_keyset) or, where the caller asked for it,
    // over a comb set's tables (k_schnorr_row_comb), one launch
    const keyset_view v = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks);
    ctx->ks_last = comb ? S2K_KEYSET_LADDER_ROW_COMB : S2K_KEYSET_LADDER_ROW;
    ctx->kg_counters = nullptr;
    ctx->last_wl_count = nullptr;
    (comb ? launch_schnorr_row_comb : launch_schnorr_row_keyset)(ctx, st, n, ks->n, (const uint32_t*)d_key_index, v.keys, v.tables, v.valid, (const uint8_t*)d_sig,
                                                                 (const uint8_t*)d_msgs, (const uint64_t*)d_msg_offsets, (uint32_t)msg_len, (uint8_t*)d_valid);
    HIP_TRY(ctx, hipGetLastError());
    return ctx_leave(ctx, st);
  }
  return schnorr_keyset_lane(ctx, ks, n, (const uint32_t*)d_key_index, (const uint8_t*)d_msgs, (const uint64_t*)d_msg_offsets, (uint32_t)msg_len,
                             (const uint8_t*)d_sig, (uint8_t*)d_valid, st);
}

// Host-buffer form: key indices, messages and signatures staged on the context's compute stream
int s2k_schnorr_verify_batch_keyset(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* key_index, const uint8_t* msgs,
                                    const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  if (n == 0) return S2K_OK;
  if (!key_index || !sig || !valid || (!msgs && (msg_offsets || msg_len))) return fail(ctx, S2K_ERR_ARG, "null buffer");
  const size_t msg_bytes = msg_offsets ? (size_t)msg_offsets[n] : n * msg_len, off_bytes = msg_offsets ? (n + 1) * 8 : 0;
  const stage_part parts[5] = {stage_in(key_index, n * 4), stage_in(msgs, msg_bytes, msg_bytes + 16), stage_in(msg_offsets, off_bytes, msg_offsets ? off_bytes : 8),
                               stage_in(sig, n * 64), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 5, n * 68 + msg_bytes, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_schnorr_verify_batch_keyset_device(c, ks, n, d[0], msgs ? d[1] : nullptr, msg_offsets ? d[2] : nullptr, msg_len, d[3], flags, d[4], st);
  });
}

// ---------------------------------------------------------------------------------------
// BIP-340 over a key set by x-only key bytes: the counterpart of s2k_ecdsa_verify_batch_keyset_bykey, with the verdicts of
// s2k_schnorr_verify_batch for the same arrays.  The caller's d_pk already holds what k_ks_expand_x would write (the challenge
// hashes, the general ladder and the worklist kernel read it in place), and the lookup is ksi_lookup32v: a key the set lists
// only as an entry that is no point is a MISS and goes through the general ladder, which lifts it - s2k_keyset_lookup_device
// with key_bytes 32 would answer that entry's index and the by-index call reject the signature.
// ---------------------------------------------------------------------------------------
static int schnorr_bykey_args(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* pk, const void* msgs, const void* msg_offsets,
                              size_t msg_len, const void* sig, uint32_t flags, const void* valid) {
  int rc = bykey_check(ctx, ks, flags);
  if (rc) return rc;
  if (flags) return fail(ctx, S2K_ERR_ARG, "s2k_schnorr_verify_batch_keyset_bykey takes no flags");
  if (n == 0) return S2K_OK;
  if (!pk || !sig || !valid || (!msgs && (msg_offsets || msg_len))) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  return S2K_OK;
}

int s2k_schnorr_verify_batch_keyset_bykey_device(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const void* d_pk, const void* d_msgs,
                                                 const void* d_msg_offsets, size_t msg_len, const void* d_sig, uint32_t flags,
                                                 void* d_valid, void* hip_stream) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = schnorr_bykey_args(ctx, ks, n, d_pk, d_msgs, d_msg_offsets, msg_len, d_sig, flags, d_valid);
  if (rc || n == 0) return rc;
  // the plain call would take k_schnorr_row or k_schnorr_quad for this n: the call IS the plain call, the set is not used
  if (bykey_delegates(ctx, n, 0)) return s2k_schnorr_verify_batch_device(ctx, n, d_pk, d_msgs, d_msg_offsets, msg_len, d_sig, 0, d_valid, hip_stream);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)hip_stream;
  rc = ctx_enter(ctx, st);
  if (rc) return rc;
  const uint8_t *pk = (const uint8_t*)d_pk, *sig = (const uint8_t*)d_sig, *msgs = (const uint8_t*)d_msgs;
  const uint64_t* offs = (const uint64_t*)d_msg_offsets;
  const uint32_t mlen = (uint32_t)msg_len;
  uint8_t* valid = (uint8_t*)d_valid;
  lane_ws w;
  rc = ks_lane_begin(ctx, ks, n, valid, st, &ctx->ks_found, &ctx->ks_found_bytes, ((n + 63) & ~(size_t)63) * sizeof(uint32_t), &w);
  if (rc) return rc;
  uint32_t* found = (uint32_t*)ctx->ks_found;
  ctx->kt_last = -1;
  const uint8_t* set_keys = s2k_internal_keyset_view(ks->base, ks->cap, ks->chunks).keys;
  // second stream: challenge hashes (over the caller's key bytes), scalars and the generator part s*G of every signature;
  // caller's: the lookup of the x-only keys among the set's valid keys, then the sort by the indices it found - a key the set
  // does not hold as a point (0xFFFFFFFF) lands in the list `left`, in the form MODE_SCHNORR_LEFT reads behind grouped_front
  // (signature indices, counted in KG_NLEFT; that ladder lifts the key itself and reads nothing else of the grouping)
  prof_mark(ctx, st, 0);
  prof_mark(ctx, st, 1);
  rc = ks_lane_fork(ctx, st);
  if (rc) return rc;
  launch_schnorr_prep(ctx->s_aux, n, w, pk, sig, msgs, offs, mlen);
  launch_generator_part(ctx, ctx->s_aux, w, 0u, (uint32_t)n);
  rc = ks_lane_launched(ctx);
  if (rc == S2K_OK) rc = keyset_index_lookup(ctx, ks, st, n, pk, S2K_KSI_X_VALID, 32, found);
  key_groups kg{};
  rc = ks_lane_sort_join(ctx, ks, n, found, st, w, rc, &kg);
  if (rc) return rc;
  prof_mark(ctx, st, 2);
  // the set's ladder over the hits (`pub`: the SET's keys - the sign flip under an odd Y; a comb set: kg.key_bytes == 64 says
  // so to MODE_SCHNORR_COMB), the general ladder over the misses with the caller's x-only keys
  launch_ladder(ctx, st, keyset_ladder_mode(ks, /*schnorr=*/true), n, 0u, set_keys, sig, w, valid, nullptr, ctx->prof_on ? ctx->clk : nullptr, kg);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 3);
  launch_ladder(ctx, st, MODE_SCHNORR_LEFT, n, 0u, pk, sig, w, valid, nullptr, nullptr, kg);
  HIP_TRY(ctx, hipGetLastError());
  launch_affine_finish(st, MODE_SCHNORR, n, (uint32_t)((n + FIN_M - 1) / FIN_M), sig, w, valid, nullptr);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 4);
  // (the worklist kernel re-does its lanes from the x-only key, hits and misses alike)
  launch_schnorr_worklist(ctx, st, n, w, pk, sig, msgs, offs, mlen, valid);
  HIP_TRY(ctx, hipGetLastError());
  prof_mark(ctx, st, 5);
  return ctx_leave(ctx, st);
}

// Host-buffer form: x-only keys, messages and signatures staged on the context's compute stream
int s2k_schnorr_verify_batch_keyset_bykey(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint8_t* pk, const uint8_t* msgs,
                                          const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig, uint32_t flags, uint8_t* valid) {
  if (!ctx) return fail(nullptr, S2K_ERR_ARG, "ctx is NULL");
  int rc = schnorr_bykey_args(ctx, ks, n, pk, msgs, msg_offsets, msg_len, sig, flags, valid);
  if (rc || n == 0) return rc;
  if (bykey_delegates(ctx, n, 0)) return s2k_schnorr_verify_batch(ctx, n, pk, msgs, msg_offsets, msg_len, sig, 0, valid);   // (with its small-call route)
  const size_t msg_bytes = msg_offsets ? (size_t)msg_offsets[n] : n * msg_len, off_bytes = msg_offsets ? (n + 1) * 8 : 0;
  const stage_part parts[5] = {stage_in(pk, n * 32), stage_in(msgs, msg_bytes, msg_bytes + 16), stage_in(msg_offsets, off_bytes, msg_offsets ? off_bytes : 8),
                               stage_in(sig, n * 64), stage_out(valid, n)};
  return s2k_internal_staged_call(ctx, parts, 5, n * 96 + msg_bytes, false, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_schnorr_verify_batch_keyset_bykey_device(c, ks, n, d[0], msgs ? d[1] : nullptr, msg_offsets ? d[2] : nullptr, msg_len, d[3], 0, d[4], st);
  });
}

// s2k_ecdsa_verify_batch_keyset without the wait at its end: the ticket's index, digest and signature arrays (100 bytes per
// signature) cross PCIe on the copy stream beside the kernels of the tickets before it; the child context verifies over
// the parent's key set.
int s2k_ecdsa_verify_batch_keyset_submit(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* key_index, const uint8_t* dig,
                                         const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* valid, s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  if (!ks || ks->ctx != ctx || ks->generation != ctx->generation || ks->device != ctx->device)
    return fail(ctx, S2K_ERR_ARG, "key set of another context");
  if (n && (!key_index || !dig || !r || !s || !valid)) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  if (flags & S2K_ECDSA_FORCE_COMPLETE) return fail(ctx, S2K_ERR_ARG, "S2K_ECDSA_FORCE_COMPLETE does not apply to key sets");
  const stage_part parts[5] = {stage_in(key_index, n * 4), stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_submit(ctx, n, valid, parts, 5, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_batch_keyset_device(c, ks, n, d[0], d[1], d[2], d[3], flags, d[4], st);
  }, ticket);
}

// s2k_schnorr_verify_batch_keyset in the ticket form (fixed-length or offset-delimited messages)
int s2k_schnorr_verify_batch_keyset_submit(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint32_t* key_index, const uint8_t* msgs,
                                           const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig, uint32_t flags, uint8_t* valid,
                                           s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  if (!ks || ks->ctx != ctx || ks->generation != ctx->generation || ks->device != ctx->device)
    return fail(ctx, S2K_ERR_ARG, "key set of another context");
  if (n && (!key_index || !sig || !valid || (!msgs && (msg_offsets || msg_len)))) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH || msg_len > 0x7fffffffu) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  if (flags) return fail(ctx, S2K_ERR_ARG, "s2k_schnorr_verify_batch_keyset takes no flags");
  const size_t msg_bytes = !n ? 0 : msg_offsets ? (size_t)msg_offsets[n] : n * msg_len, off_bytes = msg_offsets ? (n + 1) * 8 : 0;
  const stage_part parts[5] = {stage_in(key_index, n * 4), stage_in(msgs, msg_bytes, msg_bytes + 16), stage_in(msg_offsets, off_bytes, msg_offsets ? off_bytes : 8),
                               stage_in(sig, n * 64), stage_out(valid, n)};
  return s2k_internal_staged_submit(ctx, n, valid, parts, 5, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_schnorr_verify_batch_keyset_device(c, ks, n, d[0], msgs ? d[1] : nullptr, msg_offsets ? d[2] : nullptr, msg_len, d[3], 0, d[4], st);
  }, ticket);
}

// The fused calls by key bytes in the ticket form: the copies on the copy stream in front of the device form, which runs on
// the slot's child context over the parent's set and index (and, for a batch the plain call would verify on its
// wave-per-signature or four-lanes-per-signature ladder, IS the plain device call inside the ticket).
int s2k_ecdsa_verify_batch_keyset_bykey_submit(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint8_t* pub, const uint8_t* dig,
                                               const uint8_t* r, const uint8_t* s, uint32_t flags, uint8_t* valid, s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  int rc = bykey_check(ctx, ks, flags);
  if (rc) return rc;
  if (n && (!pub || !dig || !r || !s || !valid)) return fail(ctx, S2K_ERR_ARG, "null buffer");
  if (n >= S2K_MAX_BATCH) return fail(ctx, S2K_ERR_ARG, "batch too large (at most 2^30 - 1 items per call)");
  const stage_part parts[5] = {stage_in(pub, n * 64), stage_in(dig, n * 32), stage_in(r, n * 32), stage_in(s, n * 32), stage_out(valid, n)};
  return s2k_internal_staged_submit(ctx, n, valid, parts, 5, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_ecdsa_verify_batch_keyset_bykey_device(c, ks, n, d[0], d[1], d[2], d[3], flags, d[4], st);
  }, ticket);
}

int s2k_schnorr_verify_batch_keyset_bykey_submit(s2k_ctx* ctx, const s2k_keyset* ks, size_t n, const uint8_t* pk, const uint8_t* msgs,
                                                 const uint64_t* msg_offsets, size_t msg_len, const uint8_t* sig, uint32_t flags,
                                                 uint8_t* valid, s2k_ticket* ticket) {
  if (!ctx || !ticket) return fail(ctx, S2K_ERR_ARG, "null argument");
  *ticket = 0;
  int rc = schnorr_bykey_args(ctx, ks, n, pk, msgs, msg_offsets, msg_len, sig, flags, valid);
  if (rc) return rc;
  const size_t msg_bytes = !n ? 0 : msg_offsets ? (size_t)msg_offsets[n] : n * msg_len, off_bytes = msg_offsets ? (n + 1) * 8 : 0;
  const stage_part parts[5] = {stage_in(pk, n * 32), stage_in(msgs, msg_bytes, msg_bytes + 16), stage_in(msg_offsets, off_bytes, msg_offsets ? off_bytes : 8),
                               stage_in(sig, n * 64), stage_out(valid, n)};
  return s2k_internal_staged_submit(ctx, n, valid, parts, 5, [&](s2k_ctx* c, uint8_t* const* d, hipStream_t st) {
    return s2k_schnorr_verify_batch_keyset_bykey_device(c, ks, n, d[0], msgs ? d[1] : nullptr, msg_offsets ? d[2] : nullptr, msg_len, d[3], 0, d[4], st);
  }, ticket);
}

}  // extern "C"
