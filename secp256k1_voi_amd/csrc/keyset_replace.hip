// keyset_replace.hip — what s2k_keyset_replace / s2k_keyset_remove (keyset.hip) add to the table builds they share with the
// creation and the append: the host plan of a call (argument checks, the slots in ascending order, the number of pieces), the
// size of a piece, and the kernel that moves the rows of a staging set into their slots.
//   k_ks_scatter_rows   staged row j -> row slots[j] of the set: the 64 key bytes, the table row, the joint row and the
//                       validity byte.  Every section but the last is a multiple of 16 bytes at a 16-byte-aligned address and
//                       moves as uint4 per lane, a wavefront covering 1 KiB contiguous per instruction; the work is cut into
//                       tiles of KSS_TILE_QUADS quads of ONE row section, a block per tile, the grid sized by the tiles (bytes),
//                       not by the keys: one key of a JOINT6 set (a 2.75 MiB joint row) is 359 blocks, 4096 comb rows of 10 KiB are 12288
//                       tiles on the grid's cap of 2048 blocks.  No LDS; source and destination are different allocations.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <new>

#include "engine_internal.h"

using namespace s2k;

namespace {
constexpr uint32_t KSS_THREADS = 256, KSS_TILE_QUADS = KSS_THREADS * 2;   // two quads per lane: 8 KiB per block and turn
constexpr uint32_t KSS_MAX_BLOCKS = 2048;                                                         // 8 blocks per CU; the rest by grid stride
// Staging and build scratch of a call, bytes (DESIGN.md 4b "Replacing keys"): at JOINT5, the layout of the headline, 2 GiB
// are about 2300 keys = 60,000 lanes of the joint build (a lane per key and digit position), one wavefront for every SIMD of
// the chip; more keys per piece make the build no faster per key, fewer leave SIMDs idle
constexpr size_t KSS_STAGING_BUDGET = (size_t)2 << 30;
std::atomic<size_t> g_replace_piece{0};     // s2k_debug_keyset_replace_piece

struct ks_scatter_args {
  const uint4* s_keys;      // staging set: 4 quads per key ...
  uint4* d_keys;            // ... and the set
  const uint4* s_tab;       // tab_quads per key
  uint4* d_tab;
  const uint4* s_joint;     // joint_quads per key (0: the set has no joint tables)
  uint4* d_joint;
  const uint8_t* s_valid;   // a byte per key
  uint8_t* d_valid;
  const uint32_t* slots;    // staged row j goes to row slots[j] (< the set's live count: checked on the host)
  uint32_t count, tab_quads, joint_quads;
  uint32_t tab_tiles, key_tiles;   // tiles of a table row; of a whole key: 1 + tab_tiles + tiles of a joint row
};

__global__ void __launch_bounds__(KSS_THREADS) k_ks_scatter_rows(ks_scatter_args a, uint32_t total_tiles) {
  for (uint32_t t = blockIdx.x; t < total_tiles; t += gridDim.x) {
    const uint32_t j = t / a.key_tiles, sub = t - j * a.key_tiles;   // (uniform in the block)
    const size_t slot = a.slots[j];
    if (sub == 0) {
      // the key's own tile: its 64 bytes, and the validity byte as ONE byte store - its neighbours are other keys'
      if (threadIdx.x < 4) a.d_keys[slot * 4 + threadIdx.x] = a.s_keys[(size_t)j * 4 + threadIdx.x];
      else if (threadIdx.x == 4) a.d_valid[slot] = a.s_valid[j];
      continue;
    }
    const bool tab = sub <= a.tab_tiles;
    const uint32_t quads = tab ? a.tab_quads : a.joint_quads;
    const uint32_t q0 = (tab ? sub - 1 : sub - 1 - a.tab_tiles) * KSS_TILE_QUADS + threadIdx.x, q1 = q0 + KSS_THREADS;
    const uint4* __restrict__ src = (tab ? a.s_tab : a.s_joint) + (size_t)j * quads;
    uint4* __restrict__ dst = (tab ? a.d_tab : a.d_joint) + slot * quads;
    // (the loads of a row's last, partial tile read its last quad again instead of branching: both are in flight before the
    // first store waits)
    const uint4 v0 = src[q0 < quads ? q0 : quads - 1], v1 = src[q1 < quads ? q1 : quads - 1];
    if (q0 < quads) dst[q0] = v0;
    if (q1 < quads) dst[q1] = v1;
  }
}
}  // namespace

// The rows 0 .. count - 1 of the staging set (`stage`, `stage_joint`: laid out for stage_cap keys, as the set's layout is) to
// the rows d_slots[0 .. count - 1] of the set (base, joint: laid out for cap keys).  Enqueue only, on the null stream.
__attribute__((visibility("hidden"))) int s2k_internal_keyset_scatter_rows(const uint8_t* stage, size_t stage_cap, const uint4* stage_joint,
                                                                         uint8_t* base, size_t cap, uint4* joint, int jw, int chunks,
                                                                         const uint32_t* d_slots, size_t count) {
  const keyset_view s = s2k_internal_keyset_view(stage, stage_cap, chunks), d = s2k_internal_keyset_view(base, cap, chunks);
  const size_t joint_quads = joint ? s2k_internal_keyset_joint_bytes(1, jw) / sizeof(uint4) : 0;
  ks_scatter_args a{};
  a.s_keys = (const uint4*)s.keys;
  a.d_keys = (uint4*)d.keys;
  a.s_tab = s.tables;
  a.d_tab = d.tables;
  a.s_joint = stage_joint;
  a.d_joint = joint;
  a.s_valid = s.valid;
  a.d_valid = d.valid;
  a.slots = d_slots;
  a.count = (uint32_t)count;
  a.tab_quads = (uint32_t)(chunks == KC_TEETH ? KC_SLOTS : KS_SLOTS) * 8;
  a.joint_quads = (uint32_t)joint_quads;
  a.tab_tiles = (a.tab_quads + KSS_TILE_QUADS - 1) / KSS_TILE_QUADS;
  a.key_tiles = 1 + a.tab_tiles + (a.joint_quads + KSS_TILE_QUADS - 1) / KSS_TILE_QUADS;
  const uint64_t total = (uint64_t)count * a.key_tiles;
  if (count == 0 || count > stage_cap || total > 0xffffffffu) return fail(nullptr, S2K_ERR_ARG, "internal: a scatter of %zu rows", count);
  k_ks_scatter_rows<<<(unsigned)(total < KSS_MAX_BLOCKS ? total : KSS_MAX_BLOCKS), KSS_THREADS, 0, nullptr>>>(a, (uint32_t)total);
  HIP_TRY(nullptr, hipGetLastError());
  return S2K_OK;
}

// Keys per piece of a replace call over a set of this layout: what fits the staging budget - s2k_set_table_memory_budgets' cap
// where that is smaller - with the staging set's own rows and the joint build's scratch counted; at least one, and the test
// knob instead of all that when it is set
__attribute__((visibility("hidden"))) size_t s2k_internal_keyset_replace_piece(int chunks, int jw) {
  const size_t forced = g_replace_piece.load();
  if (forced) return forced;
  size_t off[5];
  const size_t fixed = s2k_internal_keyset_bytes(0, off, chunks);
  const size_t per_key = (s2k_internal_keyset_bytes(256, off, chunks) - fixed) / 256 + 1 +
                         (jw ? s2k_internal_keyset_joint_bytes(1, jw) + s2k_internal_keyset_joint_scratch_bytes(1, jw) : 0);
  size_t budget = KSS_STAGING_BUDGET;
  if (s2k_internal_keyset_budget() && s2k_internal_keyset_budget() < budget) budget = s2k_internal_keyset_budget();
  const size_t keys = budget > fixed + 1024 ? (budget - fixed - 1024) / per_key : 0;     // (1024: the sections' alignment)
  return keys ? keys : 1;
}

// The plan of a replace call, a pure host function (s2k_debug_keyset_replace_plan shows it to the tests): the arguments
// checked - every slot below n_live, none twice -, order[j] = the position in `slots` of the j-th smallest slot, and the
// number of pieces of at most piece_keys slots (0: one piece).  order and n_pieces may be null.
__attribute__((visibility("hidden"))) int s2k_internal_keyset_replace_plan(size_t n_live, size_t m, const uint32_t* slots, size_t piece_keys,
                                                                         uint32_t* order, uint64_t* n_pieces) {
  if (n_pieces) *n_pieces = 0;
  if (m == 0) return S2K_OK;
  if (!slots) return fail(nullptr, S2K_ERR_ARG, "null argument");
  if (m > n_live) return fail(nullptr, S2K_ERR_ARG, "%zu slots of a key set of %zu keys: a slot is named twice or names no key", m, n_live);
  for (size_t j = 0; j < m; ++j)
    if (slots[j] >= n_live)
      return fail(nullptr, S2K_ERR_ARG, "slot %u of a key set of %zu keys (rows behind the live ones are s2k_keyset_append's)", slots[j], n_live);
  // (slot, position) pairs sorted as 64-bit words: no indirection in the comparison (m <= n_live < 2^32)
  uint64_t* pairs = new (std::nothrow) uint64_t[m];
  if (!pairs) return fail(nullptr, S2K_ERR_NOMEM, "out of host memory");
  for (size_t j = 0; j < m; ++j) pairs[j] = (uint64_t)slots[j] << 32 | j;
  std::sort(pairs, pairs + m);
  int rc = S2K_OK;
  for (size_t j = 1; j < m && rc == S2K_OK; ++j)
    if (pairs[j] >> 32 == pairs[j - 1] >> 32) rc = fail(nullptr, S2K_ERR_ARG, "slot %u named twice in one call", (uint32_t)(pairs[j] >> 32));
  for (size_t j = 0; j < m && order; ++j) order[j] = (uint32_t)pairs[j];
  delete[] pairs;
  if (rc) return rc;
  if (n_pieces) *n_pieces = piece_keys ? (m + piece_keys - 1) / piece_keys : 1;
  return S2K_OK;
}

extern "C" {
int s2k_debug_keyset_replace_plan(size_t n_live, size_t m, const uint32_t* slots, size_t piece_keys, uint32_t* order, uint64_t* n_pieces) {
  return s2k_internal_keyset_replace_plan(n_live, m, slots, piece_keys, order, n_pieces);
}
int s2k_debug_keyset_replace_piece(size_t keys) {
  g_replace_piece.store(keys);
  return S2K_OK;
}
}  // extern "C"
