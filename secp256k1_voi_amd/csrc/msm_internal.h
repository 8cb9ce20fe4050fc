// msm_internal.h — the host interface of the multiscalar core (msm.hip), for the units that feed it: msm.hip's own plain calls,
// the whole-batch verifiers (rlc.hip), the segmented sums (msm_seg.hip) and the point sets (pointset.hip).  Nothing of the
// core's kernels is declared here; what a front end writes into the term arrays is msm_terms.h.
#pragma once
#include "engine_internal.h"

namespace {
// (in the anonymous namespace of every unit that includes this header: the core's kernels take it by value, and the profiles,
// the committed counts and tools/kernel_identity.py find those kernels by their mangled names)
struct msm_geom {
  uint32_t c;        // window bits
  uint32_t nw;       // windows = ceil(128 / c)
  uint32_t nb;       // keys per slot = 2^(c-1): the magnitudes 1 .. 2^(c-1) of a signed digit (key = magnitude - 1)
  uint32_t nslot;    // nw + 1 slots of nb keys: one per window, the top window (unsigned, up to 2^c) takes two
  uint32_t chunk_log2, nchunk;   // buckets per reduction chunk (log2), chunks per slot = nb >> chunk_log2
};
}  // namespace

// The workspace of one sum, carved out of ctx->msm_ws by msm_setup.  A front end fills scw / ptw / flag (msm_terms.h), may raise
// bits in *status, and has `aux` for itself; the rest is the core's.
struct msm_ws {
  msm_geom g;
  size_t nkeys, nslots;
  uint32_t *status, *matrix, *offset, *bsum, *scw, *ptw, *list, *sums, *xsum, *partial, *big, *lanekey;
  size_t cap;          // term capacity the workspace was carved for = plane stride of scw (a call may run on fewer terms)
  uint32_t lanes_cap;  // bucket pass: most ranges any term count up to cap can make
  size_t sum_stride;   // slots of `sums`: nkeys buckets, then the left and the right edge piece of every range
  void* pairs;
  bool wide;           // two-word pairs (term indices beyond 23 bits)
  uint32_t ncoarse, nsortblk, nblk_pad, sort_terms;
  uint8_t* flag;
  size_t zero_bytes;   // status + size bins + coarse matrix, contiguous from the start
  uint8_t* aux;        // extra caller-requested scratch
  // what msm_core's last run on this workspace cut the bucket pass into (s2k_debug_msm_terms reports them)
  uint32_t ran_L_A, ran_nlanes;   // list entries per range of the upper (or only) part; ranges of both parts
  bool ran_fold16;                // the row / column-sum reduction of the 16-bit windows
};

constexpr size_t MSM_DEBUG_TERMS_MAX = (size_t)1 << 22;     // what the test hooks lay out: 64 MiB of magnitudes, 272 MiB of records

// carve the workspace for up to n terms, + aux_bytes of scratch for the caller (force_c: 0, or the window width a test asks for at
// any size - s2k_debug_msm_terms).  Enqueues nothing; growing the workspace synchronises the device.
__attribute__((visibility("hidden"))) int msm_setup(s2k_ctx* ctx, size_t n, size_t aux_bytes, msm_ws& m, uint32_t force_c = 0);
// zero what the core counts in (status word included), on st: before the front end of every sum
__attribute__((visibility("hidden"))) hipError_t msm_clear(s2k_ctx* ctx, hipStream_t st, const msm_ws& m);
// buckets -> result: the first n terms of the workspace, filled and msm_clear'ed, summed into the 65-byte record d_out65
// (affine = false: only byte 0, identity or not, is meaningful)
__attribute__((visibility("hidden"))) int msm_core(s2k_ctx* ctx, hipStream_t st, size_t n, msm_ws& m, uint8_t* d_out65, bool affine = true);

// stage timing of the multi-scalar path (s2k_ctx_profile_msm): events before the front end (parsing, or the whole-batch
// preparation with grouping and key terms) | the sort | the bucket pass | stitching, reduction and tree | the Horner
// tail | the end
constexpr int MSM_PROF_EV = 6;
inline void msm_prof_mark(s2k_ctx* ctx, hipStream_t st, int slot) {
  if (!ctx->msm_prof_on || ctx->msm_prof_used + MSM_PROF_EV > ctx->msm_prof_cap) return;
  (void)hipEventRecord(ctx->msm_prof_ev[ctx->msm_prof_used + slot], st);
  if (slot == MSM_PROF_EV - 1) ctx->msm_prof_used += MSM_PROF_EV;
}

// One bucket-method sum of n > 0 inputs (scalars, 65-byte records) enqueued on `st` without a synchronisation; the caller has
// entered the context.  *d_status receives the address of the call's status word (non-zero after the launches: a malformed
// record), valid until the next multiscalar call of the context.  s2k_internal_msm_reserve grows the workspace to what a sum of
// n inputs needs, so that no later enqueue has to with work in flight (the carve is not monotonic in n - the window width
// changes it - so a caller reserves for every size it will run).
int s2k_internal_msm_enqueue(s2k_ctx* ctx, hipStream_t st, size_t n, const void* d_scalars, const void* d_points, void* d_out65,
                             uint32_t** d_status);
int s2k_internal_msm_reserve(s2k_ctx* ctx, size_t n);
