/*
 * secp256k1_voi_amd.h — C-ABI of the MI355X (gfx950) batch engine for the verify /
 * scalar-multiplication path of Yawning/secp256k1-voi.
 *
 * The reference is a pure-Go library with no FFI of its own; its
 * boundary is the exported Go API.  This header is what a cgo shim that keeps the
 * reference's Point / Scalar / secec.Verify surface binds to (INTEGRATION.md shows the
 * shim).  Every entry point names the reference symbol it serves (file:line relative to
 * the reference tree).
 *
 * Conventions (identical to the reference's canonical encodings):
 *   - scalars and field elements: 32-byte big-endian (Scalar.Bytes scalar.go:148,
 *     Element.Bytes field.go:151);
 *   - points, where a full point crosses the boundary: fixed 65-byte records, either
 *     0x04‖X‖Y (Point.UncompressedBytes, point_s11n.go:66) or 0x00 followed by 64 zero
 *     bytes for the identity (the reference's 1-byte identity encoding, padded);
 *   - public keys of the verify path: 64-byte X‖Y (the 65-byte SEC1 form minus the 0x04
 *     prefix, i.e. PublicKey.Bytes()[1:], secec.go:80-85);
 *   - per-item results are data (0/1 bytes), never errors — like Verify returning false
 *     (ecdsa.go:186-188).  The int return value reports infrastructure errors only.
 *   - all buffers are caller-owned; nothing is retained after a call returns.
 *   - a context is bound to one GPU and owns the device workspaces its calls share.  HOST side:
 *     calls on one context must not run concurrently (one context per goroutine/thread, like
 *     distinct receivers in the reference).  DEVICE side: the *_device entry points enqueue on
 *     the caller's stream and return without synchronising; the context chains consecutive
 *     calls with an event, so a call enqueued on another stream (or a host-buffer entry point,
 *     which uses the context's own streams) starts only after the previous call's kernels have
 *     finished — callers may switch streams freely, results are never torn.
 *
 * There is no CPU fallback: every function fails with S2K_ERR_NO_DEVICE / S2K_ERR_HIP
 * when the GPU is not usable.
 */
#ifndef SECP256K1_VOI_AMD_H
#define SECP256K1_VOI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct s2k_ctx s2k_ctx;

enum {
  S2K_OK = 0,
  S2K_ERR_NO_DEVICE = -1, /* no usable gfx950 device */
  S2K_ERR_HIP = -2,       /* a HIP runtime call failed; see s2k_last_error */
  S2K_ERR_ARG = -3,       /* null pointer / bad length / length mismatch (the reference panics: point_mul_multi.go:27) */
  S2K_ERR_NOMEM = -4,
  S2K_PENDING = 1         /* s2k_poll: the ticket is still in flight (not an error) */
};

/* flags for the ECDSA entry points */
#define S2K_ECDSA_REJECT_MALLEABLE 1u /* ECDSAOptions.RejectMalleable: reject s > n/2 (ecdsa.go:212) */
/* Diagnostics: send every signature through the complete-formula kernel that normally only
 * re-does the lanes the fast Jacobian kernel cannot decide.  Same results, ~3x slower. */
#define S2K_ECDSA_FORCE_COMPLETE 0x80000000u
/* Diagnostics: the fast ladder runs, then EVERY signature is queued for the complete-formula worklist kernel
 * (9x29 field, what decides lanes whose incomplete formulas met an exceptional case inside the ladder).  Same results,
 * ~3.4x a normal step: the price of a batch in which every lane is such a case.  The exceptional cases a key owner can
 * force for given digests - u1 G = -u2 Q (r = -e/d: decided inside the ladder kernel) and u1 G = u2 Q (r = e/d: a short
 * form of the worklist kernel, 2 u1 G) - arise in the final addition and no longer cost this; u1 = 0 needs a digest that
 * is 0 mod n.  One crafted value of u2 = r/s per ladder form used to make the ladder's last table addition add a point to
 * itself; the odd GLV split avoids it now (bench key worst_case_ladder_collision).  No input is known
 * that fills the worklist any more; the flag keeps the kernel measurable and tested. */
#define S2K_ECDSA_FORCE_WORKLIST 0x40000000u

/* bitcoin.VerifyASN1 (secec/bitcoin/ecdsa_shitcoin.go:29): BIP-0066 shape check, sighash byte
 * stripped, low-s required, 32-byte digest.  Only for s2k_ecdsa_verify_encoded_batch. */
#define S2K_ECDSA_BIP0066 2u

/* SignatureEncoding (ecdsa.go:39-53) */
#define S2K_ENCODING_ASN1 0
#define S2K_ENCODING_COMPACT 1
#define S2K_ENCODING_COMPACT_RECOVERABLE 2 /* [R | S | V], 65 bytes: ParseCompactRecoverableSignature (s11n.go:156-168) */

#define S2K_POINT_RECORD 65
#define S2K_SCALAR_SIZE 32 /* ScalarSize, scalar.go:17 */
#define S2K_COORD_SIZE 32  /* CoordSize, point_s11n.go:27-44 */

/* ---- context --------------------------------------------------------------------- */
/* Selects the device and makes the resident generator tables available (the device analogue of the package-init unpack of
 * generatorHugeAffineTable, point_mul_table.go:75-100).  The tables of a device are shared by the contexts of a process.
 * s2k_ctx_create returns as soon as a narrow table (20-bit windows, 0.8 GiB) is built - under 0.1 s - and a background
 * thread builds the wide one (26-bit windows, 40 GiB, 3 s; 24 or 22 bits when the device has less than twice that free or
 * s2k_set_generator_table_budget says so; none when even those do not fit): calls made meanwhile run on the narrow table
 * (about 2 % slower), the first CALL that starts after the build uses the wide one (a call never changes tables between its
 * launches).  Verdicts do not depend on the width.  A context's child contexts (submit / wait) use its width.
 * s2k_ctx_create_ex: gt_bits 0 = as above; 16 .. 26 = tables of exactly that width for this context, built before the call
 * returns (S2K_ERR_NOMEM when the device cannot hold them); flags S2K_CTX_WAIT_TABLES = automatic width, but return only
 * when the background build has ended.  s2k_ctx_gt_info: info[0] window bits in use now, [1] bits being aimed for (0: none),
 * [2] 1 while the build runs, [3] bytes of tables the device holds for this process; s2k_ctx_gt_note: why (free memory,
 * budget, a failed allocation); s2k_ctx_gt_wait: block until the build has ended, returns the bits in use then.
 * The builder thread is never left behind: the s2k_ctx_destroy that removes the last context of a device cancels it (it
 * looks at the flag before it allocates, between the windows of a table and before it publishes) and joins it - 0.01-0.13 s,
 * or the rest of the 40 GiB allocation when the destroy meets it (1.6 s; profiles/r06_ctx_lifecycle.txt) - and a process that
 * exits with contexts alive does the same from an atexit handler, before the HIP runtime is torn down. */
#define S2K_CTX_WAIT_TABLES 1u
int s2k_ctx_create(int device_index, s2k_ctx **out);
int s2k_ctx_create_ex(int device_index, int gt_bits, uint32_t flags, s2k_ctx **out);
void s2k_set_generator_table_budget(size_t bytes_per_device);
/* Caps for the other two table kinds of this process (0 = none): the bytes s2k_keyset_create_ex may count as free when it chooses
 * (S2K_KEYSET_AUTO) or checks a joint-table layout, and the largest per-key table buffer a verification call may allocate (a
 * larger request is treated as a failed allocation: the call degrades as it does under real memory pressure). */
void s2k_set_table_memory_budgets(size_t keyset_free_bytes, size_t key_table_bytes);
int s2k_ctx_gt_info(s2k_ctx *ctx, uint64_t info[4]);
const char *s2k_ctx_gt_note(s2k_ctx *ctx);
int s2k_ctx_gt_wait(s2k_ctx *ctx);
/* Test hook: the next s2k_ecdsa_verify_batch_device call of this (automatic) context makes the table of `bits` the one the
 * device's automatic contexts use BETWEEN its ladder launch and its worklist launch - the worst moment for the background
 * build to publish.  A call uses one table for all its launches, so its verdicts must not change.  One shot; 0 disarms. */
int s2k_debug_gt_swap_in_call(s2k_ctx *ctx, int bits);
void s2k_ctx_destroy(s2k_ctx *ctx);
const char *s2k_last_error(const s2k_ctx *ctx);
const char *s2k_version(void);
/* Compile-time configuration of this library ("GT_BITS=26 PREP_M=6 ... flags=<S2K_EXTRA_FLAGS>"),
 * so that a measurement can name the variant it ran (bench.py prints it). */
const char *s2k_build_config(void);
/* Measurement hooks (no reference counterpart; bench.py's live roofline).  While enabled, every
 * s2k_ecdsa_verify_batch_device call records HIP events on its stream around its three kernels
 * (scalar preparation, ladder, complete-formula worklist) and the ladder kernel stamps the shader
 * cycle counter against the constant-rate wall clock.  s2k_ctx_profile_read synchronises the
 * device and returns the summed durations in ms_sum3[0..2], optionally each call's ladder time
 * in ms_fast_each[0..cap), the number of calls since the last read, and the effective shader
 * clock (MHz) of the last ladder launch: shader_mhz[0] from its first wave, shader_mhz[1] from a wave
 * of its final round (the clock sags under power during a launch). */
int s2k_ctx_profile(s2k_ctx *ctx, int enable);
int s2k_ctx_profile_read(s2k_ctx *ctx, double ms_sum3[3], double *ms_fast_each, size_t cap, size_t *calls,
                         double shader_mhz[2]);
/* The same with the stages apart.  Grouping off: ms_sum5[0] scalar preparation, [2] ladder, [4]
 * complete-formula worklist.  Grouping on: [0] grouping by key, [1] per-key tables with the scalar
 * preparation running beside them, [2] ladder over the per-key tables, [3] general ladder over the
 * remaining signatures, [4] worklist.  ms_fast_each is stage [2]. */
int s2k_ctx_profile_read_stages(s2k_ctx *ctx, double ms_sum5[5], double *ms_fast_each, size_t cap, size_t *calls,
                                double shader_mhz[2]);

/* The same for the multi-scalar path (s2k_multi_scalar_mult_device, s2k_schnorr_batch_verify_rlc_device and the
 * bisection's sub-range runs): while enabled every call records HIP events on its stream between its stages;
 * s2k_ctx_profile_read_msm synchronises the device and returns the summed durations: ms_sum5[0] front end (parsing of
 * the terms; for BIP-340 the per-signature preparation with the key grouping, key lifts and key terms), [1] sort of the
 * (window, digit) keys, [2] bucket pass (k_msm_accumulate: the dominant kernel), [3] stitching of the buckets, bucket
 * reduction and tree, [4] Horner tail and affine result; and the number of calls since the last read. */
int s2k_ctx_profile_msm(s2k_ctx *ctx, int enable);
int s2k_ctx_profile_read_msm(s2k_ctx *ctx, double ms_sum5[5], size_t *calls);

/* ---- hot path: batch ECDSA verification ------------------------------------------- */
/* For each i < n: secec.PublicKey.VerifyRaw(digest, r, s) (ecdsa.go:234 -> verify :392)
 * after ParseCompactSignature's range checks (s11n.go:129-144) and NewPublicKey's point
 * validation (secec.go:188-216, point_s11n.go:178-209), all done on the device:
 *   valid[i] = 1 iff r,s in [1,n), (flags&REJECT_MALLEABLE => s <= n/2), (X,Y) canonical
 *              and on the curve, R = u1*G + u2*Q != identity and x(R) mod n == r,
 *   with e = digest32 reduced mod n (hashToScalar, ecdsa.go:477-486; the caller passes
 *   the leftmost 32 bytes of its digest).
 * Host-pointer form: copies in, runs, copies out. */
int s2k_ecdsa_verify_batch(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy /* n*64 */,
                           const uint8_t *digest32 /* n*32 */, const uint8_t *r /* n*32 */,
                           const uint8_t *s /* n*32 */, uint32_t flags, uint8_t *valid /* n */);
/* Device-pointer form: all pointers are device memory (16-byte aligned); enqueues on
 * `hip_stream` (a hipStream_t, NULL = default stream) and returns without synchronising. */
int s2k_ecdsa_verify_batch_device(s2k_ctx *ctx, size_t n, const void *d_pub_xy, const void *d_digest32,
                                  const void *d_r, const void *d_s, uint32_t flags, void *d_valid,
                                  void *hip_stream);
/* ---- signatures that share public keys ---------------------------------------------------- */
/* The reference keeps nothing per key (secec.PublicKey holds the point and its encoding, secec.go:150;
 * every Verify starts DoubleScalarMultBasepointVartime from Q, point_mul_glv.go:307).  Here a batch
 * is first grouped by public key on the device (exact: a hash table keyed by the 64 key bytes, full
 * comparison on every hit); a key with at least `min_group` signatures gets one precomputed table,
 * built inside the call, after which each of its signatures costs 12 point doublings instead of 128;
 * the other signatures take the general kernel.  Verdicts are the same either way.
 *   mode        S2K_KEYS_OFF: every signature through the general kernel (the round-1/2 path)
 *               S2K_KEYS_AUTO: as described, in every call
 *               S2K_KEYS_ALWAYS: tables even for keys with a single signature (tests)
 *               S2K_KEYS_ADAPTIVE (default): S2K_KEYS_AUTO that stops looking when there is nothing to find.  A batch
 *               whose keys never repeat pays 1-2 % for the grouping that finds nothing; the context therefore notes what
 *               each grouped call of at least 2^16 signatures found (one word written by the device into page-locked host
 *               memory, read by later calls: no synchronisation), and after two consecutive observed calls in which no
 *               key reached the threshold it verifies the next 15 such batches as S2K_KEYS_OFF does, looks again in
 *               one, and so on; the first observed call that finds a group ends the skipping.  A workload that turns
 *               from distinct keys to repeated ones is therefore verified at the general ladder's rate for up to 15
 *               calls (plus the calls already enqueued) before its tables come back.  What has been learned belongs to
 *               the context and survives mode changes; verdicts do not depend on it (s2k_ctx_key_grouping_adaptive)
 *   min_group   0 = default (4): measured break-even between 3 and 4 signatures per key
 *   hash_bits   0 = default (slots >= 2n); smaller values force probe chains (tests)
 *   max_tables  0 = default (2^22 tables of 10 KiB; the buffer is sized by the batch: n / min_group tables).  The threshold is raised until n / threshold tables
 *               fit: a batch of n signatures builds tables for keys with at least
 *               max(min_group, ceil(n / max_tables)) signatures.  A device that has no memory for the buffer does not
 *               fail the verification: the cap is halved until the buffer fits, and below 1024 tables the batch is
 *               verified without tables (same verdicts) */
#define S2K_KEYS_OFF 0
#define S2K_KEYS_AUTO 1
#define S2K_KEYS_ALWAYS 2
#define S2K_KEYS_ADAPTIVE 3
int s2k_ctx_set_key_grouping(s2k_ctx *ctx, int mode, uint32_t min_group, uint32_t hash_bits, uint32_t max_tables);
/* The tables an ECDSA or BIP-340 verification call (s2k_ecdsa_verify_batch*, s2k_schnorr_verify_batch*) builds for its
 * repeated keys, and the ladder over them.  Same verdicts either way.
 *   S2K_LADDER_COMB (default): a signed 7-tooth comb - 64 entries per key select 7 bits of a half scalar per addition:
 *               38 table additions and 18 doublings per signature (10 KiB per key)
 *   S2K_LADDER_WINDOW: odd multiples of eight 16-bit chunks, 4 bits per addition: 64 additions and 12 doublings.  Also
 *               chosen for a context created with S2K_KEYED_LADDER=window in the environment, and for any call made while
 *               S2K_KEY_TABLES_SPLIT is set.
 * Key sets have their own layouts (s2k_keyset_create_ex below; S2K_KEYSET_COMB is the comb's): this setting does not
 * touch them. */
#define S2K_LADDER_COMB 0
#define S2K_LADDER_WINDOW 1
int s2k_ctx_set_keyed_ladder(s2k_ctx *ctx, int ladder);
/* What the last s2k_ecdsa_verify_batch[_device] or s2k_schnorr_verify_batch[_device] call of the context enqueued for its
 * repeated keys: S2K_LADDER_COMB,
 * S2K_LADDER_WINDOW, or -1 when it built no tables (grouping off, a small batch, no memory).  No synchronisation. */
int s2k_ctx_last_keyed_ladder(s2k_ctx *ctx);
/* After the last s2k_ecdsa_verify_batch_device call has finished (synchronises the device):
 * stats[0] signatures verified from per-key tables, [1] tables built, [2] signatures through the
 * general kernel, [3] signatures re-done by the complete-formula kernel.  All zero after a call that took the ladders of
 * small or mid-size batches (s2k_ctx_set_small_batch_max / s2k_ctx_set_mid_batch_max) and after a key-set call that took the
 * row ladder (s2k_ctx_set_keyset_small_batch_max, s2k_ctx_set_keyset_comb_small_batch_max): they neither group nor have a
 * worklist. */
int s2k_ctx_key_grouping_stats(s2k_ctx *ctx, uint32_t stats[4]);
/* State of S2K_KEYS_ADAPTIVE, without synchronising: out[0] consecutive observed calls that found no group, [1] calls
 * still to be verified without looking, [2] calls verified without looking so far, [3] calls that looked again after a
 * run of skipped ones, [4] grouped calls whose result has been observed.  reset != 0: forget what was learned. */
int s2k_ctx_key_grouping_adaptive(s2k_ctx *ctx, uint32_t out[5], int reset);

/* ---- batch public-key recovery ------------------------------------------------------------ */
/* For each i < n: secec.RecoverPublicKey(digest, r, s, recovery_id) (ecdsa.go:244-282):
 * R = RecoverPoint(r, id) (point_s11n.go:245-282), Q = (-e/r) G + (s/r) R.  ok[i] = 1 and
 * pub65[i] = 0x04 || X || Y on success; ok[i] = 0 and a zero record when the reference returns
 * an error (r or s not in [1, n), id > 3, x = r + n not below p, x not on the curve, Q = infinity).
 * Like the reference, s > n/2 is accepted here.  flags: S2K_ECDSA_FORCE_COMPLETE only. */
int s2k_ecdsa_recover_batch(s2k_ctx *ctx, size_t n, const uint8_t *digest32 /* n*32 */, const uint8_t *r /* n*32 */,
                            const uint8_t *s /* n*32 */, const uint8_t *recovery_id /* n */, uint32_t flags,
                            uint8_t *pub65 /* n*65 */, uint8_t *ok /* n */);
int s2k_ecdsa_recover_batch_device(s2k_ctx *ctx, size_t n, const void *d_digest32, const void *d_r, const void *d_s,
                                   const void *d_recovery_id, uint32_t flags, void *d_pub65, void *d_ok,
                                   void *hip_stream);

/* ---- recoverable ECDSA signatures: the whole batch as one multi-scalar multiplication ---------- */
/* A recoverable signature (r, s, v) - ParseCompactRecoverableSignature's output (s11n.go:156-168) - names the
 * point R exactly, so a batch can be checked the way BIP-340 batches are (below): with u1_i = e_i / s_i,
 * u2_i = r_i / s_i (mod n) and R_i = RecoverPoint(r_i, v_i) (point_s11n.go:245-282),
 *   sum a_i R_i  -  (sum a_i u1_i) G  -  sum over the K distinct keys Q of (sum of a_i u2_i over Q's items) Q  ==  infinity,
 * ONE multi-scalar multiplication of n + 2K + 2 terms (a_0 = 1, a_i = 128 bits of SHA-256(key || i), key =
 * SHA-256(seed32 || 32 bytes of getrandom(2)); the items are grouped by the 64 bytes of their key on the device).
 * Item i is GOOD iff r_i, s_i in [1, n), (flags & S2K_ECDSA_REJECT_MALLEABLE => s_i <= n/2), v_i <= 3,
 * x = r_i + (v_i & 2 ? n : 0) < p and on the curve, (X_i, Y_i) canonical and on the curve (NewPublicKey,
 * secec.go:188-216), and R_i = u1_i G + u2_i Q_i for R_i = the point (x, y) with the parity of y = v_i & 1,
 * e_i = digest32 reduced mod n: secec.RecoverPublicKey(digest, r, s, v) (ecdsa.go:244-282) succeeds and returns
 * exactly the supplied key.  A good item is one VerifyRaw accepts; a plain-valid signature with the wrong v is
 * not good.  Like s2k_ecdsa_recover_batch, s > n/2 is accepted unless the flag is set.
 *   *all_valid = 1 iff every item is good (false accept probability 2^-128); n == 0: 1.
 * It does not say which item fails - s2k_ecdsa_verify_recoverable_batch_bisect does.  The reference verifies one
 * signature at a time (ecdsa.go:234).  flags: S2K_ECDSA_REJECT_MALLEABLE only; n at most 0x0fffffff.  The host-pointer
 * forms are synchronous and take turns per device like the BIP-340 ones (below). */
int s2k_ecdsa_batch_verify_rlc(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy /* n*64 */, const uint8_t *digest32 /* n*32 */,
                               const uint8_t *r /* n*32 */, const uint8_t *s /* n*32 */, const uint8_t *recovery_id /* n */,
                               uint32_t flags, const uint8_t *seed32, int *all_valid);
int s2k_ecdsa_batch_verify_rlc_device(s2k_ctx *ctx, size_t n, const void *d_pub_xy, const void *d_digest32, const void *d_r,
                                      const void *d_s, const void *d_recovery_id, uint32_t flags,
                                      const uint8_t *seed32 /* host */, int *all_valid /* host */, void *hip_stream);
/* Per-item verdicts at the price of the whole-batch check when everything is good: valid[i] = 1 iff item i is good
 * (above).  One combination over the batch; when it is rejected the failing items are located by bisection on the kept
 * terms exactly as s2k_schnorr_verify_batch_bisect does (same driver), and ranges of <= 2^17 items (or everything left,
 * once more than 8 ranges fail on one level) go through s2k_ecdsa_recover_batch_device and a comparison of the
 * recovered key with the supplied one.  stats (host, may be NULL): [0] sub-range combinations, [1] items verified
 * one by one, [2] levels descended, [3] 1 = bisection abandoned. */
int s2k_ecdsa_verify_recoverable_batch_bisect(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy, const uint8_t *digest32,
                                              const uint8_t *r, const uint8_t *s, const uint8_t *recovery_id, uint32_t flags,
                                              const uint8_t *seed32, uint8_t *valid /* n */, uint32_t stats[4]);
int s2k_ecdsa_verify_recoverable_batch_bisect_device(s2k_ctx *ctx, size_t n, const void *d_pub_xy, const void *d_digest32,
                                                     const void *d_r, const void *d_s, const void *d_recovery_id,
                                                     uint32_t flags, const uint8_t *seed32 /* host */, void *d_valid,
                                                     uint32_t stats[4] /* host */, void *hip_stream);

/* ---- key sets: per-key precomputation kept across calls ------------------------------- */
/* The reference caches per-key state in secec.PublicKey (secec/secec.go:80-85: the decoded point and its encodings,
 * built once by NewPublicKey, :188-216) and every Verify starts from it.  The device analogue: a KEY SET holds, for a
 * list of n_keys public keys (X || Y, 64 bytes each; s2k_keyset_append adds to it), the per-key tables the verification ladder otherwise
 * builds inside every call for keys that repeat in the batch (9 KiB per key; a key that is not a valid public key gets
 * a table entry marked invalid: every signature under it verifies false, as NewPublicKey would have refused the key).
 * s2k_ecdsa_verify_batch_keyset[_device]: valid[i] = PublicKey(keys[key_index[i]]).VerifyRaw(digest_i, r_i, s_i)
 * (ecdsa.go:234) with the same rules as s2k_ecdsa_verify_batch; key_index[i] >= n_keys names no key: valid[i] = 0.
 * Same verdicts as s2k_ecdsa_verify_batch on the expanded key array, bit for bit; what is saved is the grouping and the
 * table build of every call (about a third of a 2^20-signature step at 16 signatures per key).  A key set belongs to
 * the context that made it (a context destroyed and another created at the same address is NOT the owner: the set
 * remembers the context's generation and device); it may be used by any number of calls and must be destroyed before the
 * context.  Like every object of a context it is not locked: s2k_keyset_destroy / s2k_keyset_valid_keys must not run
 * while a call that uses the set is in progress on another thread. */
typedef struct s2k_keyset s2k_keyset;
int s2k_keyset_create(s2k_ctx *ctx, size_t n_keys, const uint8_t *pub_xy /* n_keys*64, host */, s2k_keyset **out);
/* The same with the table layout named.  A key set is built once, so its tables can be large:
 *   S2K_KEYSET_CHUNKS  one 8-entry chunk per 4-bit digit of a half scalar (36 KiB per key): a signature's ladder is 64 table
 *                      additions and no doubling;
 *   S2K_KEYSET_JOINT   on top of that, per digit position the sums E_a + s phi(E_b) of the chunk's entries and their images
 *                      under the endomorphism (320 KiB per key more): the two half scalars' digits at a position are ONE table
 *                      addition, 32 per signature;
 *   S2K_KEYSET_JOINT5  the same on 5-bit digits: 26 digit positions, 512 sums per position - 26 table additions per signature,
 *                      0.81 MiB per key on top of the chunk tables (56 GB for 2^16 keys);
 *   S2K_KEYSET_JOINT6  on 6-bit digits: 22 positions, 2048 sums each - 22 additions, 2.75 MiB per key (for sets of up to
 *                      2^15 keys or so on a 288 GB device);
 *   S2K_KEYSET_COMB    the signed 7-tooth comb of S2K_LADDER_COMB kept per key: 10 KiB per key and nothing else - 38 table
 *                      additions and 18 doublings per signature.  The layout for long key lists: 3.6 times smaller than
 *                      S2K_KEYSET_CHUNKS (2^22 keys: 40 GiB instead of 144).  Never chosen by S2K_KEYSET_AUTO;
 *   S2K_KEYSET_AUTO    (s2k_keyset_create) the widest of JOINT5 and JOINT that takes no more than half of the device memory
 *                      free at the time, else chunks.
 * Verdicts are identical in every layout.  s2k_keyset_layout tells which one a set has.
 * s2k_keyset_geometry (a pure host function: no device, no context) gives a layout's cost: out = {table additions per
 * signature, doublings per signature, table bytes per key}; S2K_ERR_ARG for S2K_KEYSET_AUTO and unknown layouts. */
#define S2K_KEYSET_AUTO 0
#define S2K_KEYSET_CHUNKS 1
#define S2K_KEYSET_JOINT 2
#define S2K_KEYSET_JOINT5 3
#define S2K_KEYSET_JOINT6 4
#define S2K_KEYSET_COMB 5
int s2k_keyset_create_ex(s2k_ctx *ctx, size_t n_keys, const uint8_t *pub_xy, int layout, s2k_keyset **out);
int s2k_keyset_layout(const s2k_keyset *ks);
int s2k_keyset_geometry(int layout, uint64_t out[3]);
void s2k_keyset_destroy(s2k_keyset *ks);
size_t s2k_keyset_size(const s2k_keyset *ks);
size_t s2k_keyset_device_bytes(const s2k_keyset *ks);
/* valid[k] = 1 iff key k is a valid public key (canonical coordinates, on the curve): NewPublicKey's verdict per key. */
int s2k_keyset_valid_keys(s2k_keyset *ks, uint8_t *valid /* s2k_keyset_size bytes, host */);
/* Growing a set.  A set has a CAPACITY, the number of keys its device buffers have room for, and a live count
 * (s2k_keyset_size) of keys that have tables; s2k_keyset_device_bytes is what is allocated, for the capacity.  A call's cost
 * follows the live count alone: spare capacity is memory, not time.  A key index >= s2k_keyset_size names no key (valid[i] =
 * 0), whether or not it is below the capacity.
 * s2k_keyset_create_cap: s2k_keyset_create_ex with memory for `capacity` >= n_keys keys (0: n_keys, which is what
 *   s2k_keyset_create[_ex] pass; at most 0x0fffffff).  S2K_KEYSET_AUTO chooses the layout by the bytes of the capacity.
 *   n_keys == 0 stays S2K_ERR_ARG.
 * s2k_keyset_append[_device]: n_new more keys (X || Y, 64 bytes each; host memory, or device memory of the set's device).
 *   They get the indices size .. size + n_new - 1; *first_index (may be NULL) receives the old size.  Only the tables of the
 *   new keys are built, by the kernels of the creation, in every layout; a key that is no valid public key gets a table marked
 *   invalid, as at creation.  A set with an index has the new keys inserted into it (a duplicate of an older key keeps the
 *   older index; -Q of a held Q is a second entry), so the calls by key bytes take the set's tables for them; an index that an
 *   explicit log2_slots made too small for the new count is rebuilt at the automatic size of the capacity first.  The call is
 *   synchronous and s2k_keyset_size moves only when tables and index are complete.  An append within the capacity moves no
 *   device address.  S2K_ERR_ARG when size + n_new exceeds the capacity (s2k_keyset_reserve first): the set is untouched.  A
 *   device failure leaves the size as it was, and the index without an entry for a row that did not become a key (or, when
 *   that cannot be had either, the set without an index).  n_new == 0: S2K_OK.
 * s2k_keyset_reserve: memory for `capacity` keys.  Synchronises the device, allocates, copies every section of the set and its
 *   joint tables device to device and frees the old buffers after the copies.  Both copies exist for a moment: a set that
 *   fills more than half of the free device memory (2^16 keys at S2K_KEYSET_JOINT5 are 56 GB) cannot grow this way -
 *   S2K_ERR_NOMEM, the set intact - and should be given its capacity at creation.  capacity <= s2k_keyset_capacity: S2K_OK, nothing changes.  The
 *   index is rebuilt when it has fewer than 2 * capacity slots.
 * Threading: as s2k_keyset_destroy and s2k_keyset_index_create - no call or ticket that uses the set may be in progress. */
int s2k_keyset_create_cap(s2k_ctx *ctx, size_t n_keys, const uint8_t *pub_xy, int layout, size_t capacity, s2k_keyset **out);
size_t s2k_keyset_capacity(const s2k_keyset *ks);
int s2k_keyset_reserve(s2k_keyset *ks, size_t capacity);
int s2k_keyset_append(s2k_keyset *ks, size_t n_new, const uint8_t *pub_xy /* n_new*64, host */, uint32_t *first_index /* may be NULL */);
int s2k_keyset_append_device(s2k_keyset *ks, size_t n_new, const void *d_pub_xy /* n_new*64 */, uint32_t *first_index);
/* Replacing and removing keys in place.  s2k_keyset_replace[_device] overwrites the live rows slots[0 .. m-1] of a set with the
 * keys pub_xy[0 .. m-1] (X || Y, 64 bytes each; host memory, or device memory of the set's device - `slots` is host memory in
 * both forms).  THE CONTRACT: after a successful call the set behaves, bit for bit, like a set created whole with
 * s2k_keyset_create_cap from the key list K' of the same layout and capacity, K'[slots[j]] = pub_xy[j] and every other row
 * unchanged - in every call that takes a set (by index, by key bytes, encoded, ECDSA and BIP-340, small and large, every
 * layout), in s2k_keyset_valid_keys, in s2k_keyset_lookup* and in the occupied count of s2k_keyset_index_info.  A signature
 * whose key index names a replaced row is verified under the new key.  A duplicate of the old key elsewhere in the set takes
 * over the lookup's answer for those bytes, and a new key that duplicates a held one answers with the lower of the two rows:
 * the index is built anew over the live rows, at the number of slots and with the seed it has.
 * s2k_keyset_remove is s2k_keyset_replace with 64 zero bytes per slot.  (0, 0) is no point of the curve: the row is what
 *   NewPublicKey (secec.go:188-216) would have refused - its validity byte 0, every signature under it false, never an answer
 *   of the 33-byte and valid-x-only lookups (the 64-byte lookup of 64 zero bytes finds it, as it finds any row by its bytes).
 * s2k_keyset_size, s2k_keyset_capacity and every other row's index are unchanged; no device address moves.  The library keeps
 * no list of free slots: which rows are free to be reused is the caller's bookkeeping (an LRU, epochs, ...).
 * Cost: the tables of the m keys - built, m at a time up to a bounded piece, in a staging set (at most 2 GiB, or the cap of
 *   s2k_set_table_memory_budgets where that is smaller; a piece is at least one key) and moved to their rows by one copy kernel
 *   per piece - and the index build.  The launches follow the pieces, not m and not how scattered the slots are.  The device
 *   form reads its m * 64 key bytes back once (the pairs are sorted by slot on the host).
 * S2K_ERR_ARG, before anything is touched: a NULL argument with m > 0; a slot >= s2k_keyset_size (the rows size .. capacity - 1
 *   are s2k_keyset_append's); the same slot twice in one call.  m == 0: S2K_OK.
 * Failure: everything the call allocates (staging, build scratch, the new index table) is allocated before the first byte of
 *   the set changes, so S2K_ERR_NOMEM leaves the set exactly as it was.  A device failure once rows are being written leaves
 *   the rows named by the call undefined; the index is then built over the rows as they are, and a set whose index cannot be
 *   rebuilt keeps its tables and loses its index (s2k_keyset_index_create makes another).
 * Threading and ordering: as s2k_keyset_append - synchronous, on the null stream, the device idle before and after; not beside
 *   a call or ticket that uses the set. */
int s2k_keyset_replace(s2k_keyset *ks, size_t m, const uint32_t *slots /* m, host */, const uint8_t *pub_xy /* m*64, host */);
int s2k_keyset_replace_device(s2k_keyset *ks, size_t m, const uint32_t *slots /* m, HOST */, const void *d_pub_xy /* m*64 */);
int s2k_keyset_remove(s2k_keyset *ks, size_t m, const uint32_t *slots /* m, host */);
/* Test hooks of the above, pure host functions.  s2k_debug_keyset_replace_plan: the argument checks and the order a call with
 * these slots over a set of n_live keys works in - S2K_ERR_ARG as the call; order[j] (m words, may be NULL) = the position in
 * `slots` of the j-th smallest slot; *n_pieces (may be NULL) = the pieces of at most piece_keys slots (0: one piece).
 * s2k_debug_keyset_replace_piece: every later call of the process works in pieces of `keys` keys (0: the automatic size). */
int s2k_debug_keyset_replace_plan(size_t n_live, size_t m, const uint32_t *slots, size_t piece_keys, uint32_t *order /* m */,
                                  uint64_t *n_pieces);
int s2k_debug_keyset_replace_piece(size_t keys);
/* Test hook: the tables of key `key` of a set read back, entries first .. first + count - 1 of one section, into `out` (host
 * memory).  Synchronous, on the null stream; the calling rules of s2k_keyset_valid_keys (not beside a call that uses the set).
 * Every table entry of a key is a point m * Q of the key Q on the key's isomorphic curve: for the affine (x, y) of m * Q what
 * is stored is (W^2 x, W^3 y), and where there is a third column beta W^2 x, with W the one Z all entries of the key share.
 * Limb-stored entries are read with the loaders of the ladders (ke_load*, je_load) and fully reduced; every coordinate is 32
 * big-endian bytes.
 *   section 0, the shared scale: count must be 1; out = 32 bytes, W (element W_SLOT of the window geometry's scratch, element
 *     W of entry WENT of a comb set).
 *   section 1, the base table: 96 bytes per entry, X || Y || beta X - but for the lead pair, which has no beta column (no
 *     ladder takes the endomorphism of a starting point): its last 32 bytes are zero.  S2K_KEYSET_CHUNKS, _JOINT, _JOINT5, _JOINT6: the
 *     32-chunk table, 258 entries - entry 8 c + a = (2 a + 1) 16^c Q for c < 32, a < 8, then the lead pair L + phi(L),
 *     L - phi(L) with L = 2^128 Q at 256 and 257.  S2K_KEYSET_COMB: 66 entries - E[idx] = B_6 + sum_{t<6} (2 idx_t - 1) B_t,
 *     B_t = 2^(19 t) Q, for idx < 64, then the lead pair from L = 2^115 Q.
 *   section 2, the joint table: 64 bytes per entry, X || Y.  S2K_KEYSET_JOINT: 4096 entries, entry 128 c + 2 (8 a + b) + s =
 *     E_a + (-1)^s phi(E_b), E_a = (2 a + 1) 16^c Q.  S2K_KEYSET_JOINT5 / _JOINT6 (W = 5 / 6 bits, POS = 26 / 22 positions,
 *     NE = 16 / 32 odd multiples): POS * 2 NE^2 + 2 entries, entry 2 NE^2 i + 2 (NE a + b) + s = (2 a + 1) B_i +
 *     (-1)^s phi((2 b + 1) B_i), B_i = 2^(W i) Q, then the lead pair 2^(W POS) Q +- phi(2^(W POS) Q).  A wide entry comes as
 *     the eight 32-bit words per coordinate it is stored as, most significant first and NOT reduced: the ladder takes them
 *     for canonical, and a test is what checks that.  S2K_KEYSET_CHUNKS and _COMB have no section 2.
 * S2K_ERR_ARG, `out` untouched and nothing launched: a NULL argument; key >= s2k_keyset_size; a section the layout does not
 * have; first + count beyond the section; count != 1 in section 0.  count == 0 (sections 1 and 2): S2K_OK.  The rows of a key
 * that is no valid public key are returned as they are: their content is unspecified. */
int s2k_debug_keyset_entries(s2k_keyset *ks, size_t key, int section, size_t first, size_t count, uint8_t *out /* host */);
/* The entries section `section` of the set's layout has (1 / 258 or 66 / 4096, 13314 or 45058), a pure host function:
 * S2K_ERR_ARG, *entries untouched, for a NULL argument or a section the layout does not have. */
int s2k_debug_keyset_section_entries(const s2k_keyset *ks, int section, size_t *entries);
int s2k_ecdsa_verify_batch_keyset(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint32_t *key_index /* n */,
                                  const uint8_t *digest32, const uint8_t *r, const uint8_t *s, uint32_t flags, uint8_t *valid);
int s2k_ecdsa_verify_batch_keyset_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_key_index /* n uint32 */,
                                         const void *d_digest32, const void *d_r, const void *d_s, uint32_t flags,
                                         void *d_valid, void *hip_stream);

/* ---- key sets by key bytes: device index, lookup and a fused ECDSA call -------------------- */
/* The calls above want every signature's key as an INDEX into the set; what a caller has is key bytes (the reference's shape
 * is PublicKey.Verify(digest, sig), and every ingest path of this library produces key bytes).  The INDEX of a key set maps
 * key bytes to key indices on the device: an open-addressing hash table over the set's keys (8 bytes per slot), hashed under
 * a seed drawn per set from the operating system, every hit confirmed against all the bytes of the set's key.  The caller
 * owns the set and decides that it has an index; nothing builds one implicitly, and a call by key bytes over a set without
 * one is S2K_ERR_ARG.  Keys of the set that are no valid public keys are indexed like any other: a hit on one verifies false,
 * which is what s2k_ecdsa_verify_batch answers under such a key.  A set that lists a key several times answers with the
 * LOWEST of its indices.
 *
 * s2k_keyset_index_geometry (host only: no device, no context): out = {slots, bytes of the index}; log2_slots 0 = auto, the
 *   power of two >= 2 * n_keys, at least 16 (s2k_keyset_index_create with log2_slots 0 takes it for the set's CAPACITY; an
 *   explicit log2_slots is checked against the keys there are).  S2K_ERR_ARG when 2^log2_slots <= n_keys, log2_slots > 31, or n_keys is 0 or
 *   > 0x0fffffff.
 * s2k_keyset_index_create builds the index of a set (an allocation of its own, NOT counted in s2k_keyset_device_bytes;
 *   s2k_keyset_index_info tells its size).  Same threading rule as s2k_keyset_destroy.  A set has at most one index: a
 *   second call is S2K_ERR_ARG.  Freed by s2k_keyset_destroy.
 * s2k_keyset_index_info: out = {slots (0: the set has no index), bytes, occupied slots = distinct 64-byte keys of the set,
 *   longest probe distance of a stored entry}.
 * s2k_keyset_lookup[_device]: key_index[i] = the lowest index of a key of the set equal to the key_bytes bytes at
 *   keys + i * stride (key_bytes 64: X || Y; 32: X alone - the x-only key of BIP-340, which stands for Q and -Q alike, as
 *   s2k_schnorr_verify_batch_keyset defines it), else 0xFFFFFFFF.  stride >= key_bytes: 65-byte SEC1 records are looked
 *   up from their second byte with stride 65 (no alignment is asked for).  Exact: never a false miss, never a false hit.
 *   key_bytes 33: SEC1 compressed keys, prefix || X (stride >= 33).  key_index[i] = what key_bytes 64 gives for the point
 *   the 33 bytes decode to (SetCompressedBytes, point_s11n.go:140-176), and 0xFFFFFFFF when they decode to nothing (a prefix
 *   other than 02 / 03, X >= p, X^3 + 7 not a square) or the set does not hold that point.  No square root is taken: the
 *   answer is the set's VALID key (s2k_keyset_valid_keys) with this X and a Y of the asked parity - there is at most one
 *   such point, so it is the decoded one; an off-curve (X, Y') of the same parity that the set lists too is never answered.
 *   Every other key_bytes is S2K_ERR_ARG.
 *   The device form only enqueues; its output feeds s2k_ecdsa_verify_batch_keyset_device /
 *   s2k_schnorr_verify_batch_keyset_device on the same stream, which treat 0xFFFFFFFF as "no key": invalid.
 * s2k_ecdsa_verify_batch_keyset_bykey[_device]: valid[i] = what s2k_ecdsa_verify_batch gives for the same arrays, bit for
 *   bit.  Signatures whose key the set holds run on the set's tables (every layout), the others on the general ladder from
 *   the key bytes supplied - NOT on tables built inside the call: a batch that mostly misses the set should use
 *   s2k_ecdsa_verify_batch.  The device form is enqueued without a host synchronisation (lookup, sort, both ladders and the
 *   complete-formula worklist in stream order); the host form stages 160 bytes per signature.
 *   When s2k_ecdsa_verify_batch would take its wave-per-signature or four-lanes-per-signature ladder for this n (n at most
 *   s2k_ctx_set_small_batch_max / s2k_ctx_set_mid_batch_max, grouping mode ADAPTIVE or OFF, no S2K_ECDSA_FORCE_WORKLIST), the
 *   call IS s2k_ecdsa_verify_batch[_device] on the supplied arrays and the set is not used (s2k_ctx_key_grouping_stats reads
 *   all zero afterwards).  Otherwise s2k_ctx_key_grouping_stats gives [0] signatures whose key the set holds, [1] 0,
 *   [2] signatures on the general ladder, [3] the complete-formula worklist.
 *   S2K_ERR_ARG: a set of another context or device, a set without an index, S2K_ECDSA_FORCE_COMPLETE.  n == 0: S2K_OK.
 *   S2K_ECDSA_REJECT_MALLEABLE and S2K_ECDSA_FORCE_WORKLIST are honoured.
 * s2k_schnorr_verify_batch_keyset_bykey[_device]: the BIP-340 counterpart.  pk: n x-only keys of 32 bytes; messages and
 *   signatures as s2k_schnorr_verify_batch takes them (msgs NULL with msg_len 0 and no offsets: empty messages).  valid[i] =
 *   what s2k_schnorr_verify_batch gives for the same arrays, bit for bit, in every layout of the set.  A signature runs on the
 *   set's tables when the set holds a VALID key (s2k_keyset_valid_keys) with its X - of either parity of Y: the key stands
 *   for lift_x(X) -, and otherwise on the general ladder, which lifts the key bytes supplied.
 *   Invalid set entries: a key the set lists only as an entry that is no point (X, Y' off the curve; a coordinate >= p) counts
 *   as a miss, wherever a real (X, Y) stands in the list; the key then goes through the general ladder and may verify.  This
 *   is where the call differs from s2k_keyset_lookup_device with key_bytes 32 in front of
 *   s2k_schnorr_verify_batch_keyset_device: that lookup answers the lowest index of ANY entry with this X, so the two-call
 *   route rejects a signature under a key whose lowest entry is invalid, and rejects every key outside the set (0xFFFFFFFF is
 *   "no key" there), where s2k_schnorr_verify_batch verifies them.  The fused call also reads the caller's key bytes in
 *   place, where the by-index call first expands n * 32 bytes of keys from the set.
 *   Delegation: the rule of the ECDSA call.  When s2k_schnorr_verify_batch_device would take its wave-per-signature or
 *   four-lanes-per-signature ladder for this n (n at most s2k_ctx_set_small_batch_max / s2k_ctx_set_mid_batch_max, grouping
 *   mode ADAPTIVE or OFF), the call IS s2k_schnorr_verify_batch[_device] on the supplied arrays, the set is not used and
 *   s2k_ctx_key_grouping_stats reads all zero afterwards.  Otherwise s2k_ctx_key_grouping_stats gives [0] signatures on the
 *   set's tables, [1] 0, [2] signatures on the general ladder, [3] the complete-formula worklist.
 *   flags must be 0: S2K_ECDSA_FORCE_COMPLETE is S2K_ERR_ARG as for every key-set call, and so is every other flag.
 *   S2K_ERR_ARG as well: a set of another context or device, a set without an index, n >= 2^30, msg_len > 0x7fffffff.
 *   n == 0: S2K_OK, no buffer is touched.  The device form is enqueued without a host synchronisation; the host form stages
 *   keys, messages, offsets and signatures on the context's compute stream.
 * s2k_ecdsa_verify_batch_keyset_bykey_submit, s2k_schnorr_verify_batch_keyset_bykey_submit: the ticket forms (s2k_wait,
 *   s2k_poll, s2k_wait_all; the rules of s2k_ecdsa_verify_batch_submit for the buffers).  The ticket runs the device form over
 *   the context's set and index; a batch the rule above delegates runs the plain device call inside the ticket.
 * Not provided: group forms of the fused calls, a BIP-340 form of the encoded call (s2k_ecdsa_verify_encoded_batch_keyset),
 * removing keys of a set. */
int s2k_keyset_index_geometry(size_t n_keys, uint32_t log2_slots, uint64_t out[2]);
int s2k_keyset_index_create(s2k_keyset *ks, uint32_t log2_slots);
int s2k_keyset_index_info(const s2k_keyset *ks, uint64_t out[4]);
int s2k_keyset_lookup(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *keys, size_t key_bytes, size_t stride,
                      uint32_t *key_index);
int s2k_keyset_lookup_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_keys, size_t key_bytes, size_t stride,
                             void *d_key_index, void *hip_stream);
int s2k_ecdsa_verify_batch_keyset_bykey(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pub_xy, const uint8_t *digest32,
                                        const uint8_t *r, const uint8_t *s, uint32_t flags, uint8_t *valid);
int s2k_ecdsa_verify_batch_keyset_bykey_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_pub_xy,
                                               const void *d_digest32, const void *d_r, const void *d_s, uint32_t flags,
                                               void *d_valid, void *hip_stream);
int s2k_schnorr_verify_batch_keyset_bykey(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pk /* n*32 */,
                                          const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                                          const uint8_t *sig /* n*64 */, uint32_t flags, uint8_t *valid);
int s2k_schnorr_verify_batch_keyset_bykey_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_pk, const void *d_msgs,
                                                 const void *d_msg_offsets, size_t msg_len, const void *d_sig, uint32_t flags,
                                                 void *d_valid, void *hip_stream);

/* Page-locked host buffers for the host-pointer entry points (no reference counterpart: the reference never leaves the
 * host; this is the price of the boundary, cf. secec.PublicKey.Verify, ecdsa.go:171-228, which a cgo shim batches into
 * s2k_ecdsa_verify_batch).  From pageable memory every copy is staged by the runtime and 2^20 verifications cost
 * 8.4-9.5 ms against 5.2-5.7 resident; from pinned memory the copies are asynchronous and the batch is processed in one
 * grouped call whose table phase overlaps the transfer of the digests and signatures.  s2k_host_alloc / s2k_host_free:
 * hipHostMalloc / hipHostFree (NULL on failure).  s2k_host_register / s2k_host_unregister: pin memory the caller
 * already owns; unregister before the memory is freed or moved.  The buffer must start on a page boundary and cover
 * whole pages (S2K_ERR_ARG otherwise): the runtime pins and unmaps pages, and a block of the C or Go heap shares its
 * first and last page with its neighbours - on ROCm 7.2 a later pageable copy from such a re-used page takes the
 * process down with a GPU memory access fault.  Memory from mmap / aligned_alloc(page, k * page) qualifies; a Go
 * slice does not (take the buffers from s2k_host_alloc instead).
 * s2k_ecdsa_verify_batch detects pinned buffers by itself (all four inputs must be pinned). */
void *s2k_host_alloc(size_t bytes);
void s2k_host_free(void *p);
int s2k_host_register(void *p, size_t bytes);
int s2k_host_unregister(void *p);

/* ---- submit / wait: the host-pointer entry points without the wait at their end ------------ */
/* The reference's caller has its data in host memory (secec.PublicKey.Verify, ecdsa.go:171-228) and a cgo shim batches
 * it into s2k_ecdsa_verify_batch, which pays the PCIe transfer and the kernels in series (7.1 ms from pinned, 8.2 ms
 * from pageable memory against 4.9 ms resident per 2^20 signatures).  s2k_ecdsa_verify_batch_submit returns as soon as
 * the batch is enqueued (from page-locked buffers: at once; from pageable ones: when the runtime has staged the copies)
 * and s2k_wait blocks until the verdicts of that ticket are in `valid`.  The context keeps up to FOUR batches in flight on
 * internal child contexts (own workspaces on the same device; the generator tables are shared), in two lanes: even and odd
 * tickets run on two sets of streams beside each other, within a lane the kernels of consecutive tickets follow each other,
 * and a ticket crosses PCIe while its lane's previous ticket computes - a caller that keeps three or four batches
 * submitted sees a little more than the resident rate of a single stream.  A fifth submit first retires the oldest ticket
 * (delivers its verdicts; a later s2k_wait on it returns at once).  s2k_poll is s2k_wait without the blocking: S2K_PENDING while the
 * ticket is in flight.  Same verdicts as s2k_ecdsa_verify_batch, bit for bit; the inputs and `valid` must
 * stay untouched until the ticket has been waited for (or retired).  Submit, wait and the other calls of one context
 * must come from one thread at a time, like all calls on a context; the key-grouping settings are those the context
 * has at submit time.  s2k_wait_all retires everything in flight (oldest first; s2k_ctx_destroy does the same).
 * Each child holds what s2k_ctx_device_bytes reports minus the generator tables. */
typedef uint64_t s2k_ticket;
int s2k_ecdsa_verify_batch_submit(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy, const uint8_t *digest32, const uint8_t *r,
                                  const uint8_t *s, uint32_t flags, uint8_t *valid, s2k_ticket *ticket);
int s2k_wait(s2k_ctx *ctx, s2k_ticket ticket);
int s2k_poll(s2k_ctx *ctx, s2k_ticket ticket);
int s2k_wait_all(s2k_ctx *ctx);
/* Small batches.  A call of up to a few thousand signatures leaves the device empty whatever it runs, and costs the latency
 * of ONE signature's ladder; for batches of up to max_n items (default 3072; 0 = never) s2k_ecdsa_verify_batch,
 * s2k_schnorr_verify_batch and s2k_ecdsa_recover_batch (and their _device / _submit forms) therefore run ladders that spend
 * a whole wavefront on each item (k_verify_row / k_schnorr_row / k_recover_row: the row arithmetic of fe29r.h, complete
 * formulas), and the synchronous host forms move their bytes without DMA transfers (the CPU copies them into a page-locked
 * block the kernels read and write in place): host to host 0.20 instead of 0.74 ms for 1024 ECDSA signatures, 0.19 instead of
 * 0.83 for BIP-340, 0.24 instead of 0.87 for recovery - the reference's own shape is a loop of single PublicKey.Verify calls (secec/ecdsa.go:171; BASELINE config 1
 * verifies 1024).  Same results (tests/test_gpu_round5.py::test_small_batch_*).  A grouping mode set by name
 * (S2K_KEYS_AUTO / S2K_KEYS_ALWAYS) is obeyed at every size; the default (S2K_KEYS_ADAPTIVE) and S2K_KEYS_OFF take these
 * ladders. */
int s2k_ctx_set_small_batch_max(s2k_ctx *ctx, uint32_t max_n);
/* Batches above that threshold and up to max_n items (default 32768; 0 = never) run ladders with FOUR lanes per signature
 * (k_verify_quad / k_schnorr_quad / k_recover_quad, pt29q.h): calls of this size fill neither kind of kernel, and what they cost
 * is the latency of one wave's ladder - half as long this way as with a lane per signature (0.35 instead of 0.6-0.7 ms for
 * 2^12 .. 2^14 ECDSA signatures).  Same results (tests/test_gpu_round5.py). */
int s2k_ctx_set_mid_batch_max(s2k_ctx *ctx, uint32_t max_n);
/* Small calls over a key set.  s2k_ecdsa_verify_batch_keyset and s2k_schnorr_verify_batch_keyset (and their _device / _submit
 * forms) of up to max_n signatures (default 2048, the measured crossover; 0 = never) run ONE launch with a wavefront per signature over the 32-chunk
 * table of the signature's key (k_verify_row_keyset / k_schnorr_row_keyset: 64 complete additions on the key's isomorphic
 * curve - b3 = 21 W^6 is a per-key field element there, pt29r_add_b3 -, then the generator part), instead of the chain of
 * launches and the lane-per-signature ladder of larger calls.  Sets of layout S2K_KEYSET_CHUNKS, JOINT, JOINT5 and JOINT6
 * take it (all keep the chunk table); S2K_KEYSET_COMB sets have a threshold of their own (below); calls with
 * S2K_ECDSA_FORCE_WORKLIST keep the lane-per-signature path.  Same verdicts (tests/test_gpu_keyset_row.py). */
int s2k_ctx_set_keyset_small_batch_max(s2k_ctx *ctx, uint32_t max_n);
/* Small calls over a COMB key set, opt-in.  The same calls over an S2K_KEYSET_COMB set of up to max_n signatures (default 0 =
 * never: such calls keep the lane-per-signature path unless the caller asks) run ONE launch with a wavefront per signature
 * over the comb table of the signature's key (k_verify_row_comb / k_schnorr_row_comb).  A comb entry (x, y), affine on the
 * key's isomorphic curve, is the projective point (x W : y : W^3) of secp256k1 - one product layer for the two entries of a
 * column -, so the ladder runs on secp256k1 itself with no per-key constant: 37 complete additions, 18 doublings and 19
 * conversions, 166 product layers against the chunk table's 257, then the generator part.  The by-index calls only; calls
 * with S2K_ECDSA_FORCE_WORKLIST keep the lane-per-signature path.  Same verdicts (tests/test_gpu_keyset_comb_row.py). */
int s2k_ctx_set_keyset_comb_small_batch_max(s2k_ctx *ctx, uint32_t max_n);
/* What the last key-set verification call of the context enqueued: S2K_KEYSET_LADDER_LANE (a lane per signature),
 * S2K_KEYSET_LADDER_ROW (a wavefront per signature on a chunk table), S2K_KEYSET_LADDER_ROW_COMB (a wavefront per signature
 * on a comb table), -1 before any.  No synchronisation. */
#define S2K_KEYSET_LADDER_LANE 0
#define S2K_KEYSET_LADDER_ROW 1
#define S2K_KEYSET_LADDER_ROW_COMB 2
int s2k_ctx_last_keyset_ladder(s2k_ctx *ctx);
/* Times of a ticket on the device's clock, for placement diagnostics (s2k_group_member_stats_ex): after
 * s2k_ctx_ticket_timing(ctx, 1) every submitted ticket records three moments on the device's clock: t0 = its first host-to-device
 * copy is about to start, t1 = its last copy has ended, t2 = its verdicts are in host memory.  t0 <= t1 <= t2 by construction
 * (the stream that delivers the verdicts waits for the marker behind the copies), also when several contexts share the
 * device's hardware queues.  s2k_ticket_times gives ms[0] = t1 - t0 (the copies), ms[1] = t2 - t0 (first copy to verdicts), so
 * 0 < ms[0] <= ms[1], for one of the last eight retired tickets (S2K_PENDING and zeros otherwise). */
int s2k_ctx_ticket_timing(s2k_ctx *ctx, int enable);
int s2k_ticket_times(s2k_ctx *ctx, s2k_ticket ticket, double ms[2]);
/* s2k_ecdsa_verify_batch_keyset in the same form: signatures that name their key by its index in a key set of this context
 * (100 bytes per signature cross PCIe instead of 160, and no table is built).  Tickets of all submit entry points share
 * the context's four slots and may be mixed.  The key set has to live until the ticket has been waited for (s2k_keyset_destroy
 * waits for the device first, so destroying it early blocks rather than breaks). */
int s2k_ecdsa_verify_batch_keyset_submit(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint32_t *key_index,
                                         const uint8_t *digest32, const uint8_t *r, const uint8_t *s, uint32_t flags,
                                         uint8_t *valid, s2k_ticket *ticket);
/* The fused calls by key bytes (s2k_ecdsa_verify_batch_keyset_bykey, s2k_schnorr_verify_batch_keyset_bykey: "key sets by key
 * bytes" above) in the same form: the set needs its index, 160 bytes per ECDSA signature and 96 + the message per BIP-340
 * signature cross PCIe, and a batch the fused call delegates runs the plain device call inside the ticket. */
int s2k_ecdsa_verify_batch_keyset_bykey_submit(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pub_xy,
                                               const uint8_t *digest32, const uint8_t *r, const uint8_t *s, uint32_t flags,
                                               uint8_t *valid, s2k_ticket *ticket);
int s2k_schnorr_verify_batch_keyset_bykey_submit(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pk /* n*32 */,
                                                 const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                                                 const uint8_t *sig /* n*64 */, uint32_t flags, uint8_t *valid, s2k_ticket *ticket);
/* s2k_ecdsa_verify_encoded_batch (below) in the same form */
int s2k_ecdsa_verify_encoded_batch_submit(s2k_ctx *ctx, size_t n, const uint8_t *pubs, const uint64_t *pub_off,
                                          const uint8_t *digests, const uint64_t *dig_off, const uint8_t *sigs,
                                          const uint64_t *sig_off, int encoding, size_t digest_len, uint32_t flags,
                                          uint8_t *valid, s2k_ticket *ticket);

/* ---- several devices in one process ------------------------------------------------------------ */
/* north_star: "batches shard trivially across the 8 GPUs of one node".  A Go process cannot be one rank of a
 * torch.distributed job; in ONE process no collective is needed at all.  A GROUP owns one context and one host thread per
 * listed device (a device may be listed more than once: two members then share it, each with its own context).  A batch
 * is cut into contiguous index shards, one per member (signature i belongs to shard i * members / n
 * up to rounding to 256), every member runs s2k_ecdsa_verify_batch_submit / s2k_wait on its shard from its own thread,
 * and the verdicts land in the caller's `valid` at the shard's offset - the "all-gather" is the host array itself.
 * Verdicts are those of s2k_ecdsa_verify_batch on the whole batch, bit for bit (signatures are independent; only the
 * grouping by key is per shard).  s2k_group_ecdsa_verify_batch = submit + wait.  Up to four group batches are in flight
 * per member (a fifth submit blocks until the oldest is done).  Listing a device twice is for tests: two members then run
 * four lanes on it, which is slower than one member's two.  Group calls may come from any ONE thread at a time.
 * s2k_device_count: devices visible to the runtime (0 when there is none). */
typedef struct s2k_group s2k_group;
int s2k_device_count(void);
/* Host topology of a device (topology.cpp; sysfs, S2K_SYSFS_ROOT replaces "/sys"): its PCI bus id ("0000:05:00.0"), the NUMA
 * node it hangs off (-1: unknown, single-node machines included), and the two actions built on it: restrict the CALLING
 * thread to the CPUs of a node that it may run on (returns how many, 0 = nothing changed; never widens the mask), prefer
 * a node for a range of pages (0 = done or nothing to do, -1 = refused).  s2k_topology_*: the parsers, with the sysfs
 * root as an argument (NULL: the default). */
int s2k_device_pci_bus_id(int device, char *out, size_t len /* >= 13 */);
int s2k_device_numa_node(int device);
int s2k_bind_thread_to_node(int node);
int s2k_topology_prefer_node(void *p, size_t bytes, int node);
int s2k_topology_node_count(const char *sysfs_root);
int s2k_topology_numa_node_of_pci(const char *sysfs_root, const char *bus_id);
int s2k_topology_node_cpus(const char *sysfs_root, int node, int *cpus, size_t cap);
int s2k_group_create(const int *devices, size_t n_devices, s2k_group **out);
/* ... with the members' generator table width and context flags as s2k_ctx_create_ex takes them (0, 0 = s2k_group_create) */
int s2k_group_create_ex(const int *devices, size_t n_devices, int gt_bits, uint32_t flags, s2k_group **out);
void s2k_group_destroy(s2k_group *g);
size_t s2k_group_size(const s2k_group *g);
const char *s2k_group_last_error(const s2k_group *g);
int s2k_group_set_key_grouping(s2k_group *g, int mode, uint32_t min_group, uint32_t hash_bits, uint32_t max_tables);
int s2k_group_set_small_batch_max(s2k_group *g, uint32_t max_n);   /* s2k_ctx_set_small_batch_max on every member (a member's shard is what counts as the batch) */
int s2k_group_set_mid_batch_max(s2k_group *g, uint32_t max_n);     /* s2k_ctx_set_mid_batch_max on every member */
int s2k_group_set_keyset_small_batch_max(s2k_group *g, uint32_t max_n);   /* s2k_ctx_set_keyset_small_batch_max on every member */
int s2k_group_set_keyset_comb_small_batch_max(s2k_group *g, uint32_t max_n);   /* s2k_ctx_set_keyset_comb_small_batch_max on every member */
int s2k_group_ecdsa_verify_batch(s2k_group *g, size_t n, const uint8_t *pub_xy, const uint8_t *digest32, const uint8_t *r,
                                 const uint8_t *s, uint32_t flags, uint8_t *valid);
int s2k_group_ecdsa_verify_batch_submit(s2k_group *g, size_t n, const uint8_t *pub_xy, const uint8_t *digest32,
                                        const uint8_t *r, const uint8_t *s, uint32_t flags, uint8_t *valid, s2k_ticket *ticket);
int s2k_group_wait(s2k_group *g, s2k_ticket ticket);
/* s2k_ecdsa_verify_encoded_batch (below) across the group: the three blobs are shared, every member takes a contiguous range of
 * ITEMS (its slice of the offset arrays; the offsets stay absolute). */
int s2k_group_ecdsa_verify_encoded_batch(s2k_group *g, size_t n, const uint8_t *pubs, const uint64_t *pub_off,
                                         const uint8_t *digests, const uint64_t *dig_off, const uint8_t *sigs,
                                         const uint64_t *sig_off, int encoding, size_t digest_len, uint32_t flags, uint8_t *valid);
int s2k_group_ecdsa_verify_encoded_batch_submit(s2k_group *g, size_t n, const uint8_t *pubs, const uint64_t *pub_off,
                                                const uint8_t *digests, const uint64_t *dig_off, const uint8_t *sigs,
                                                const uint64_t *sig_off, int encoding, size_t digest_len, uint32_t flags,
                                                uint8_t *valid, s2k_ticket *ticket);
/* stats[m * 4 + 0..3] for member m, of its last finished shard: signatures, first index, milliseconds from the member's
 * submit to its verdicts (host clock), device index. */
int s2k_group_member_stats(s2k_group *g, double *stats /* 4 * members */);
/* The same and more, stats[m * 8 + 0..7]: signatures, first index, host milliseconds, device index, NUMA node of the device
 * (-1 unknown), CPUs the member's thread is bound to (0: not bound), and of the last finished shard [6] the milliseconds of its
 * host-to-device copies and [7] the milliseconds from its first copy to its verdicts, on the device's clock as
 * s2k_ticket_times defines them: 0 < [6] <= [7] for every member, whatever shares its device (the first call switches that
 * timing on: zero until a shard has been submitted after it).  Placement: every member's thread binds itself
 * to the CPUs of its device's NUMA node (sysfs; no-op on one node, when the node is unknown or the cpuset forbids it). */
int s2k_group_member_stats_ex(s2k_group *g, double *stats /* 8 * members */);
/* Blocks until the wide generator tables of every member's device are in (s2k_ctx_gt_wait per member); returns the smallest
 * window width in use.  For benchmarks and services that want their full rate from the first batch. */
int s2k_group_gt_wait(s2k_group *g);
/* Items per member of a batch of n: member i takes [i * size, min(n, (i + 1) * size)). */
size_t s2k_group_shard_size(const s2k_group *g, size_t n);
/* A page-locked array of n items of bytes_per_item bytes laid out for the group: the pages of every member's shard are
 * placed on the NUMA node of that member's device (first touched there; mbind where the kernel allows), so that on a
 * two-socket node no device pulls its shard across the socket link.  One node / unknown nodes: an ordinary pinned block.
 * NULL on failure (s2k_group_last_error).  Freed by s2k_group_host_free or with the group.  The reference keeps its data on
 * the Go heap (secec/ecdsa.go:171-228), which cannot be pinned (s2k_host_register above): a cgo shim fills these instead. */
void *s2k_group_host_alloc(s2k_group *g, size_t bytes_per_item, size_t n);
void s2k_group_host_free(s2k_group *g, void *p);
/* BASELINE configs 3 and 4 across a group (synchronous; the multi-process forms are sharding.py's).  The BIP-340 whole-batch
 * check: every member checks its contiguous shard as one random linear combination (s2k_schnorr_batch_verify_rlc; the
 * members' coefficients are independent: every call mixes fresh operating-system randomness into the seed), *all_valid = 1
 * iff every shard is accepted.  The multiscalar multiplication: every member sums its shard of the terms, the first member
 * adds the partial sums.  Same results as the single-context calls (Point.MultiScalarMultVartime, point_mul_multi.go:73-117: variable time). */
int s2k_group_schnorr_batch_verify_rlc(s2k_group *g, size_t n, const uint8_t *pk /* n*32 */, const uint8_t *msgs,
                                       const uint64_t *msg_offsets, size_t msg_len, const uint8_t *sig /* n*64 */,
                                       const uint8_t *seed32, int *all_valid);
int s2k_group_multi_scalar_mult(s2k_group *g, size_t n, const uint8_t *k /* n*32 */, const uint8_t *points /* n*65 */,
                                uint8_t *out65);
/* Key sets across a group: every member builds the tables of all n_keys keys on its own device (side by side; the
 * tables are replicated per device like the generator tables: s2k_group_keyset_device_bytes per member), and
 * s2k_group_ecdsa_verify_batch_keyset[_submit] shards a batch of (key index, digest, r, s) items like any other group
 * call, each member verifying its shard over its own copy (s2k_ecdsa_verify_batch_keyset_submit).  Same verdicts as
 * s2k_ecdsa_verify_batch_keyset on one device.  The set belongs to its group and is destroyed before it; tickets are those
 * of s2k_group_wait.  What secec.PublicKey caches per key (secec/secec.go:80-85), for a stable key set, on every GPU of the node. */
typedef struct s2k_group_keyset s2k_group_keyset;
int s2k_group_keyset_create(s2k_group *g, size_t n_keys, const uint8_t *pub_xy /* n_keys*64, host */, int layout,
                            s2k_group_keyset **out);
void s2k_group_keyset_destroy(s2k_group_keyset *gks);
size_t s2k_group_keyset_size(const s2k_group_keyset *gks);
int s2k_group_keyset_layout(const s2k_group_keyset *gks);
size_t s2k_group_keyset_device_bytes(const s2k_group_keyset *gks);
/* s2k_keyset_create_cap, s2k_keyset_reserve and s2k_keyset_append on every member's set, on the members' threads.  The first
 * failing member's code is returned; members that had succeeded keep the keys appended (their sets are then longer than the
 * group's), and s2k_group_keyset_size moves only when every member succeeded.  No group call that uses the set may be in
 * progress. */
int s2k_group_keyset_create_cap(s2k_group *g, size_t n_keys, const uint8_t *pub_xy, int layout, size_t capacity,
                                s2k_group_keyset **out);
size_t s2k_group_keyset_capacity(const s2k_group_keyset *gks);
int s2k_group_keyset_reserve(s2k_group_keyset *gks, size_t capacity);
int s2k_group_keyset_append(s2k_group_keyset *gks, size_t n_new, const uint8_t *pub_xy /* n_new*64, host */, uint32_t *first_index);
/* s2k_keyset_replace / s2k_keyset_remove on every member's set (host keys), on the members' threads; the size does not move.
 * A refusal is every member's, before anything is touched; the first failing member's code is returned. */
int s2k_group_keyset_replace(s2k_group_keyset *gks, size_t m, const uint32_t *slots /* m, host */, const uint8_t *pub_xy /* m*64, host */);
int s2k_group_keyset_remove(s2k_group_keyset *gks, size_t m, const uint32_t *slots /* m, host */);
int s2k_group_ecdsa_verify_batch_keyset(s2k_group *g, const s2k_group_keyset *gks, size_t n, const uint32_t *key_index,
                                        const uint8_t *digest32, const uint8_t *r, const uint8_t *s, uint32_t flags,
                                        uint8_t *valid);
int s2k_group_ecdsa_verify_batch_keyset_submit(s2k_group *g, const s2k_group_keyset *gks, size_t n, const uint32_t *key_index,
                                               const uint8_t *digest32, const uint8_t *r, const uint8_t *s, uint32_t flags,
                                               uint8_t *valid, s2k_ticket *ticket);

/* Packs valid[n] (0/1 bytes, device) into a bitmap (bit i of byte i/8, LSB first; (n+7)/8
 * bytes, device) and writes the number of valid items to *d_count (uint64, device).  This is
 * the payload of the multi-GPU bitmap all-gather (the count travels behind the bitmap shard). */
int s2k_pack_valid_device(s2k_ctx *ctx, size_t n, const void *d_valid, void *d_bitmap, void *d_count,
                          void *hip_stream);
/* Bytes of the per-signature device workspace (tables, scratch, worklist) for batches of up to n signatures.  It is
 * ONE of the context's buffers: see s2k_ctx_device_bytes for everything a verification call of n signatures holds. */
size_t s2k_ecdsa_workspace_bytes(size_t n);
/* Device memory the context holds once it has verified a batch of n signatures with its current key-grouping
 * settings (s2k_ctx_set_key_grouping): the resident generator tables (40 GiB), the per-signature workspace above, and -
 * with the grouping on, the default, for n >= 256 - the grouping arrays and the per-key table buffer (n / min_group
 * tables of 9 KiB, at most max_tables: 2.4 GB at n = 2^20, 38 GB at 2^24, whether or not keys repeat).  The multi-scalar and BIP-340
 * batch entry points keep a workspace of their own on top (about 1.4 KB per term), and the verification calls that take
 * messages (s2k_ecdsa_verify_messages_batch*) a digest buffer of 32 n bytes, allocated on the first such call: neither is
 * counted here, and what this function returns for given settings is what it always returned.  Size HBM by this, not by
 * s2k_ecdsa_workspace_bytes alone, when several contexts share a device. */
size_t s2k_ctx_device_bytes(const s2k_ctx *ctx, size_t n);

/* ---- host-side ingest: the reference's byte-level parsing, in batch --------------------- */
/* ParseASN1Signature (secec/s11n.go:83): strict DER SEQUENCE { r INTEGER, s INTEGER }, r, s in
 * [1, n).  Returns 0 and fills r, s (32-byte big-endian); 1 = malformed ASN.1
 * (errInvalidAsn1Sig); 2 = scalar out of range (errInvalidScalar).  Pure host code. */
int s2k_parse_asn1_signature(const uint8_t *der, size_t len, uint8_t r[32], uint8_t s[32]);
/* ParseCompactSignature (secec/s11n.go:129): [R | S], 64 bytes.  Same return codes. */
int s2k_parse_compact_signature(const uint8_t *sig, size_t len, uint8_t r[32], uint8_t s[32]);
/* bitcoin.IsValidSignatureEncodingBIP0066 (secec/bitcoin/asn1_shitcoin.go:13): 1 / 0. */
int s2k_is_valid_signature_encoding_bip0066(const uint8_t *sig_with_sighash, size_t len);
/* PublicKey.Verify(digest, sig, opts) (secec/ecdsa.go:171) for n encoded items: SEC1 public
 * keys (33 or 65 bytes, as secec.NewPublicKey accepts, secec.go:188), digests, and signatures
 * in `encoding`, each as a concatenation with n+1 byte offsets.  digest_len = 0 means
 * opts == nil (any digest of >= 32 bytes); otherwise digests of another length verify false
 * (ecdsa.go:184-188).  flags: S2K_ECDSA_REJECT_MALLEABLE, S2K_ECDSA_BIP0066,
 * S2K_ECDSA_FORCE_COMPLETE.  The bytes are uploaded as they are; parsing, decompression of
 * compressed keys and verification all run on the device.  valid[i] is the bool the
 * reference's Verify returns; keys it could not even construct give 0.
 * encoding S2K_ENCODING_COMPACT_RECOVERABLE (ecdsa.go:204-205,220-226): the key is recovered from (digest, r, s, v) on
 * the verification ladder (RecoverPublicKey, ecdsa.go:244-282) and compared with the supplied one on the device
 * (PublicKey.Equal: the serialised points, secec.go:121-129); RejectMalleable applies before the recovery (ecdsa.go:212).
 * s2k_ecdsa_verify_encoded_batch_submit: the same without the wait at the end (s2k_wait; see
 * s2k_ecdsa_verify_batch_submit).
 * PRECONDITION on the three offset arrays, of this call, its _submit form and the two key-set forms below: offsets never
 * decrease (off[i] <= off[i + 1] for every i < n), and off[n] is the size of the blob in bytes (off[0] need not be 0: the
 * bytes before it are not read).  The calls do NOT verify this: no scan of the 3 (n + 1) offsets is made.  A decreasing
 * offset makes an item's length, and the byte count of a workgroup's stretch, wrap around: the device then reads outside
 * the blob.  The caller must check offsets that come from an untrusted source. */
int s2k_ecdsa_verify_encoded_batch(s2k_ctx *ctx, size_t n, const uint8_t *pubs, const uint64_t *pub_off,
                                   const uint8_t *digests, const uint64_t *dig_off, const uint8_t *sigs,
                                   const uint64_t *sig_off, int encoding, size_t digest_len, uint32_t flags,
                                   uint8_t *valid);
/* s2k_ecdsa_verify_encoded_batch over a key set with an index (s2k_keyset_index_create): valid[i] = what
 * s2k_ecdsa_verify_encoded_batch gives for the same arguments, bit for bit, in every layout of the set.  The parse step
 * resolves each SEC1 key against the set's index: a 65-byte key as s2k_keyset_lookup with key_bytes 64 does, a 33-byte key
 * as key_bytes 33 does - a compressed key the set holds is replaced by the set's own 64 bytes and costs NO square root.
 * Compressed keys the set does not hold are collected in a list, and only that list is decompressed (densely: a batch with
 * one such key per wave pays for list / 64 waves of roots, not for all of them).  Signatures whose key the set holds run on
 * its tables, the others on the general ladder, as in s2k_ecdsa_verify_batch_keyset_bykey.
 * encoding: S2K_ENCODING_ASN1 or S2K_ENCODING_COMPACT; flags: S2K_ECDSA_REJECT_MALLEABLE, S2K_ECDSA_BIP0066 and
 * S2K_ECDSA_FORCE_WORKLIST are honoured.  S2K_ERR_ARG: S2K_ENCODING_COMPACT_RECOVERABLE (it recovers the key and has no use
 * for a set), S2K_ECDSA_FORCE_COMPLETE, a set without an index, a set of another context or device.  n == 0: S2K_OK.
 * The synchronous call works in pieces whose copies overlap the previous piece's kernels.  A piece the plain call would
 * verify on its wave-per-signature or four-lanes-per-signature ladder (the rule of s2k_ecdsa_verify_batch_keyset_bykey) is
 * parsed and verified exactly as s2k_ecdsa_verify_encoded_batch does, without the set; a call that is one such piece IS
 * that call.  s2k_ctx_key_grouping_stats afterwards, of the LAST piece: [0] signatures that parsed and whose key the set
 * holds, [1] 0, [2] signatures on the general ladder, [3] the complete-formula worklist.
 * _submit: one ticket (s2k_wait), the whole batch in one piece, as s2k_ecdsa_verify_encoded_batch_submit; the set must stay
 * alive until the ticket has been waited for.
 * s2k_ctx_last_encoded_keyset_stats synchronises and gives, summed over the pieces of the context's last SYNCHRONOUS call:
 * [0] signatures verified under a key of the set that came as 33 bytes, [1] as 65 bytes, [2] the length of the
 * decompression list = square roots taken, [3] items of the pieces the set was not used for. */
int s2k_ecdsa_verify_encoded_batch_keyset(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pubs, const uint64_t *pub_off,
                                          const uint8_t *digests, const uint64_t *dig_off, const uint8_t *sigs,
                                          const uint64_t *sig_off, int encoding, size_t digest_len, uint32_t flags,
                                          uint8_t *valid);
int s2k_ecdsa_verify_encoded_batch_keyset_submit(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pubs,
                                                 const uint64_t *pub_off, const uint8_t *digests, const uint64_t *dig_off,
                                                 const uint8_t *sigs, const uint64_t *sig_off, int encoding, size_t digest_len,
                                                 uint32_t flags, uint8_t *valid, s2k_ticket *ticket);
int s2k_ctx_last_encoded_keyset_stats(s2k_ctx *ctx, uint64_t out[4]);
/* Test hooks for the parse step of the encoded calls (ingest.hip).
 * s2k_debug_parse_encoded runs, for the piece [first, first + cnt) of a batch of n_total items, the kernels the encoded calls
 * run in front of their ladders - through the same launch helpers -, and no ladder: ks NULL: k_parse_encoded; else (a set with
 * an index, as s2k_ecdsa_verify_encoded_batch_keyset asks) k_parse_encoded_keyset, k_decompress_list,
 * k_decompress_list_close.  Blobs, offsets (n_total + 1 each), encoding, digest_len and flags as the encoded calls take them
 * (S2K_ECDSA_BIP0066 implies 32-byte digests and low-s there as here); the piece's bytes go up where the offsets say.  Every
 * output is filled with `sentinel` on the device before the launch and copied back whole afterwards, so the caller sees which
 * rows were written: xy[n_total * 64], dg / r / s[n_total * 32], recid[n_total] (S2K_ENCODING_COMPACT_RECOVERABLE only, else
 * NULL), and with a set found[cnt] (key index per item of the piece), list[cnt] (the decompression list: its first
 * counters[3] entries are items of the batch, in no fixed order) and counters[8]: the call's four counters {hits of 33-byte
 * keys, of 65-byte keys, roots of the pieces before, length of the list} read after k_decompress_list, then again after
 * k_decompress_list_close.  new_call != 0 zeroes the counters first, as the start of a call does; 0 goes on counting: a
 * second piece of the same call.  Unlike the encoded calls, the hook scans the offsets and refuses decreasing ones.
 * Synchronous; uses the context's buffers and counters (s2k_ctx_last_encoded_keyset_stats reads them), so not for use beside
 * calls in flight.
 * s2k_debug_parse_encoded_caps: out = the bytes of LDS the parse kernels stage a workgroup's stretch of the key, digest and
 * signature blob in; a stretch from lo to hi is staged when (hi - (lo & ~15)) + 16 <= the capacity, else read in place. */
int s2k_debug_parse_encoded(s2k_ctx *ctx, const s2k_keyset *ks, size_t n_total, const uint8_t *pubs, const uint64_t *pub_off,
                            const uint8_t *digests, const uint64_t *dig_off, const uint8_t *sigs, const uint64_t *sig_off,
                            size_t first, size_t cnt, int encoding, size_t digest_len, uint32_t flags, int new_call,
                            uint8_t sentinel, uint8_t *xy, uint8_t *dg, uint8_t *r, uint8_t *s, uint8_t *recid, uint32_t *found,
                            uint32_t *list, uint32_t counters[8]);
int s2k_debug_parse_encoded_caps(uint32_t out[3]);

/* ---- BIP-340 Schnorr verification (batched) ---------------------------------------- */
/* For each i < n: bitcoin.SchnorrPublicKey.Verify(msg_i, sig_i) for the x-only key pk_i
 * (secec/bitcoin/schnorr.go:221-253): valid[i] = 1 iff pk_i is a valid x-only key
 * (NewSchnorrPublicKey, :257-275), r < p, s < n, and R = s*G - e*P is finite with even y and
 * x(R) == r, e = tagged hash "BIP0340/challenge" of r || pk || msg reduced mod n (:420-449),
 * computed on the device.  Messages: either n strings of msg_len bytes each (msg_offsets ==
 * NULL) or concatenated with msg_offsets[n+1] byte offsets (any lengths, as the reference
 * allows).  flags: S2K_ECDSA_FORCE_COMPLETE only. */
int s2k_schnorr_verify_batch(s2k_ctx *ctx, size_t n, const uint8_t *pk /* n*32 */, const uint8_t *msgs,
                             const uint64_t *msg_offsets, size_t msg_len, const uint8_t *sig /* n*64 */,
                             uint32_t flags, uint8_t *valid /* n */);
int s2k_schnorr_verify_batch_device(s2k_ctx *ctx, size_t n, const void *d_pk, const void *d_msgs,
                                    const void *d_msg_offsets, size_t msg_len, const void *d_sig, uint32_t flags,
                                    void *d_valid, void *hip_stream);
/* The same for signatures that name their key by its index in a key set of this context (s2k_keyset_create[_ex]: X || Y keys).
 * BIP-340's public key is the x coordinate and its point lift_x(x), the one with even y (NewSchnorrPublicKeyFromPoint,
 * schnorr.go:276-300, does that to a point): key k of the set stands for the x-only key X_k whatever the parity of its Y.
 * valid[i] = SchnorrPublicKey(X of keys[key_index[i]]).Verify(msg_i, sig_i); an index outside the set, or a key that is no
 * point of the curve: 0.  Same verdicts as s2k_schnorr_verify_batch on the expanded x-only keys, bit for bit, in every
 * layout of the set; no grouping, key lift or table build per call.  flags: 0. */
int s2k_schnorr_verify_batch_keyset(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint32_t *key_index /* n */,
                                    const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                                    const uint8_t *sig /* n*64 */, uint32_t flags, uint8_t *valid);
int s2k_schnorr_verify_batch_keyset_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_key_index,
                                           const void *d_msgs, const void *d_msg_offsets, size_t msg_len, const void *d_sig,
                                           uint32_t flags, void *d_valid, void *hip_stream);
/* ... and as a ticket of the context's submit / wait slots (s2k_wait / s2k_poll / s2k_wait_all, above) */
int s2k_schnorr_verify_batch_keyset_submit(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint32_t *key_index,
                                           const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                                           const uint8_t *sig, uint32_t flags, uint8_t *valid, uint64_t *ticket);

/* Whole-batch BIP-340 verification as ONE multi-scalar multiplication of n + K + 1 points
 * ((sum a_i s_i) G - sum a_i R_i - sum over the K distinct keys P of (sum of a_i e_i over P's signatures) P
 * == infinity, a_0 = 1, a_i = 128 bits of SHA-256(key || i), key = SHA-256(seed32 || 32 bytes of
 * getrandom(2)); the signatures are grouped by key on the device).  *all_valid = 1 iff every
 * signature of the batch verifies (false accept probability 2^-128).  seed32 should be fresh CSPRNG
 * output; because the library mixes in operating-system randomness of its own, a reused or
 * predictable seed does not make the coefficients predictable.  It does not say which signature
 * fails — s2k_schnorr_verify_batch_bisect does.  The
 * reference has single verification only (schnorr.go:221); this is BASELINE config 4.
 * A refused call (S2K_ERR_ARG: a NULL buffer, n >= 2^28, msg_len >= 2^31 - in both forms before anything is staged
 * or launched) leaves *all_valid = 0. */
/* (Host-pointer forms of the whole-batch calls - this one, s2k_schnorr_verify_batch_bisect, s2k_multi_scalar_mult - are
 * synchronous: transfer, kernels, answer.  Two contexts on two host threads that take whole batches alternately overlap one's
 * transfer with the other's kernels; the library makes the phases of such calls take turns per device, so the two settle at
 * about the resident rate instead of falling into lock step.) */
int s2k_schnorr_batch_verify_rlc(s2k_ctx *ctx, size_t n, const uint8_t *pk, const uint8_t *msgs,
                                 const uint64_t *msg_offsets, size_t msg_len, const uint8_t *sig,
                                 const uint8_t *seed32, int *all_valid);
int s2k_schnorr_batch_verify_rlc_device(s2k_ctx *ctx, size_t n, const void *d_pk, const void *d_msgs,
                                        const void *d_msg_offsets, size_t msg_len, const void *d_sig,
                                        const uint8_t *seed32 /* host */, int *all_valid /* host */, void *hip_stream);

/* Per-signature BIP-340 verdicts at the price of the whole-batch check when everything verifies
 * (the usual case): one combination over the batch; when it is rejected, the failing signatures
 * are located by bisection — the lifted points, challenges and coefficients of the whole batch are
 * kept, a half-range is re-checked as a multiscalar multiplication of its own terms, the other
 * half's error point follows by subtraction, and ranges of <= 2^17 signatures (or everything left,
 * once more than 8 ranges fail on one level) go through s2k_schnorr_verify_batch.  valid[i] is
 * what SchnorrPublicKey.Verify returns for item i (schnorr.go:221-253), up to a false accept
 * probability of 2^-128 per combination.  stats (host, may be NULL): [0] sub-range combinations,
 * [1] signatures verified one by one, [2] levels descended, [3] 1 = bisection abandoned. */
int s2k_schnorr_verify_batch_bisect(s2k_ctx *ctx, size_t n, const uint8_t *pk, const uint8_t *msgs,
                                    const uint64_t *msg_offsets, size_t msg_len, const uint8_t *sig,
                                    const uint8_t *seed32, uint8_t *valid, uint32_t stats[4]);
int s2k_schnorr_verify_batch_bisect_device(s2k_ctx *ctx, size_t n, const void *d_pk, const void *d_msgs,
                                           const void *d_msg_offsets, size_t msg_len, const void *d_sig,
                                           const uint8_t *seed32 /* host */, void *d_valid, uint32_t stats[4] /* host */,
                                           void *hip_stream);

/* ---- group operations (batched; host pointers) -------------------------------------
 * VARIABLE TIME, like everything that runs on the GPU here: these serve the reference's *Vartime
 * code paths (public scalars: verification, recovery, batch checks).  They must NOT be bound to
 * Point.ScalarMult / Point.ScalarBaseMult, which the reference keeps constant-time for ECDH and
 * signing (point_mul_glv.go:257, point_mul_table.go:168): those are served by the s2k_ct_*
 * functions below, on the host CPU. */
/* out[i] = k[i]*G — scalarBaseMultVartime (point_mul_table.go:197) */
int s2k_scalar_base_mult_batch(s2k_ctx *ctx, size_t n, const uint8_t *k /* n*32 */, uint8_t *out /* n*65 */);
/* out[i] = k[i]*P[i] — scalarMultVartimeGLV (point_mul_glv.go:203) */
int s2k_scalar_mult_batch(s2k_ctx *ctx, size_t n, const uint8_t *k, const uint8_t *points /* n*65 */, uint8_t *out);
/* out[i] = u1[i]*G + u2[i]*P[i] — Point.DoubleScalarMultBasepointVartime (point_mul_glv.go:307) */
int s2k_double_scalar_mult_basepoint_batch(s2k_ctx *ctx, size_t n, const uint8_t *u1, const uint8_t *u2,
                                           const uint8_t *points, uint8_t *out);
/* The same two operations with an implementation selector (for the parity tests, which run the
 * reference's vectors through BOTH implementations; the entry points above use S2K_IMPL_FAST):
 *   S2K_IMPL_COMPLETE  the reference's algorithm shape: complete projective formulas on the 8x32
 *                      field (what k_verify_fallback runs for lanes the ladder cannot decide);
 *   S2K_IMPL_FAST      the verification ladder itself (k_verify_fast: 9x29 lazy field, common-Z
 *                      odd-multiple table, signed odd digits of the odd GLV split, Jacobian
 *                      doublings / mixed additions, resident generator tables) with undecided
 *                      lanes re-done by the complete path, exactly as in a verification.
 * u1 == NULL: out[i] = u2[i]*P[i] (scalarMultVartimeGLV).  A record that is neither 0x04||X||Y on
 * the curve nor the identity record gives S2K_ERR_ARG (the reference cannot construct such Points). */
#define S2K_IMPL_COMPLETE 0u
#define S2K_IMPL_FAST 1u
int s2k_double_scalar_mult_basepoint_batch_ex(s2k_ctx *ctx, uint32_t impl, size_t n, const uint8_t *u1,
                                              const uint8_t *u2, const uint8_t *points, uint8_t *out);
/* out[i] = a[i] + b[i] — Point.Add (point.go:62); out[i] = 2*a[i] — Point.Double (point.go:71) */
int s2k_point_add_batch(s2k_ctx *ctx, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out);
int s2k_point_double_batch(s2k_ctx *ctx, size_t n, const uint8_t *a, uint8_t *out);
/* out = sum_i k[i] * P[i] — Point.MultiScalarMultVartime (point_mul_multi.go:73-117) ONLY: variable time
 * (data-dependent bucket sorts).  The constant-time Point.MultiScalarMult (:25-67) binds to
 * s2k_ct_multi_scalar_mult below, never to this.  n == 0 gives the identity.  Pippenger bucket method with
 * complete additions (the reference uses Straus; same group element).  A malformed point
 * record is S2K_ERR_ARG.  The device form takes device pointers and synchronises the stream
 * before returning (it has to read back the status word). */
int s2k_multi_scalar_mult(s2k_ctx *ctx, size_t n, const uint8_t *k /* n*32 */, const uint8_t *points /* n*65 */,
                          uint8_t *out /* 65 */);
int s2k_multi_scalar_mult_device(s2k_ctx *ctx, size_t n, const void *d_k, const void *d_points, void *d_out65,
                                 void *hip_stream);
/* Test hook for the bucket method (the core of msm.hip) behind the call above, the segmented sums and both whole-batch
 * verifiers (rlc.hip): out = sum_i +-mag[i] * P[i]
 * over nterms TERMS as the parse and split kernels would have left them - mags: 16 bytes each, big-endian, the whole range
 * 0 .. 2^128 - 1 (the halves of the endomorphism split stay below 0xA2A9 * 2^112; only the raw coefficients of the whole-batch
 * checks go beyond); points: 65-byte records 0x04 || X || Y of points on the curve, or all zero for an identity term (flag 0:
 * the term is skipped); signs: NULL, or one byte per term, non-zero negates the point.  window_bits 0: the width the call chooses for
 * nterms terms; 8, 12 or 16: that width at any size.  A small kernel of the hook fills the term arrays (msm_store_term), then
 * the sort, the bucket pass, the reduction and the tail run as in the product.  geom[10] = {c, nw, nb, nslot, nkeys, L_A,
 * nlanes, fold16, big, list_len}: window bits, windows, keys per slot, slots, keys (padded to a multiple of 256), list
 * entries per range of the bucket pass and ranges, and 1 when the 16-bit reduction by row and column sums ran (these three are
 * the core's own values, as the call ran them, not a restatement; in the two-part flow of S2K_MSM_SPLIT_WINDOW L_A is the
 * upper part's and nlanes counts the ranges of both parts), the count of buckets spread over more than 8 ranges (k_msm_stitch's counter:
 * it goes beyond the 4096 the queue holds) and the length of the sorted list.  offsets / list: both NULL, or offsets[nkeys_cap]
 * with nkeys_cap >= nkeys + 1 and list[list_cap] with list_cap >= list_len: the sort's offset[0 .. nkeys] and list[0 ..
 * list_len) (term index | 0x80000000 for a negative digit; key = window * nb + |digit| - 1; the order inside a key is not
 * defined).  S2K_ERR_ARG: nterms == 0 or above 2^22, another window_bits, a point record that is neither, buffers too small.
 * Synchronous; uses the context's multiscalar workspace, so not for use beside calls in flight. */
int s2k_debug_msm_terms(s2k_ctx *ctx, size_t nterms, const uint8_t *mags /* nterms*16 */, const uint8_t *points /* nterms*65 */,
                        const uint8_t *signs /* nterms or NULL */, int window_bits, uint8_t *out /* 65 */, uint32_t geom[10],
                        uint32_t *offsets, size_t nkeys_cap, uint32_t *list, size_t list_cap);
/* Test hooks for the two whole-batch verifiers (s2k_schnorr_batch_verify_rlc, s2k_ecdsa_batch_verify_rlc and their bisect
 * calls): the ERROR POINT of a batch under a coefficient key that is taken as given.  key32 IS the PRF key of the
 * coefficients (a_0 = 1, a_i = the low 128 bits of SHA-256(key32 || i as 8 bytes, big-endian)) - where the product derives it
 * as SHA-256(seed32 || getrandom), these take it from the caller and no operating-system randomness enters, so the result is
 * an exact, predictable group element: E = sum of a_i E_i over the items that are in the combination, with
 *   BIP-340   E_i = s_i G - lift_x(r_i) - e_i lift_x(pk_i)
 *   ECDSA     E_i = R_i - u1_i G - u2_i Q_i   (as s2k_ecdsa_batch_verify_rlc states it),
 * the identity exactly for an item the per-signature call accepts.  NOT for production: a known key makes the check forgeable.
 * form 0, the aggregated form: what the whole-batch calls run (keys grouped on the device under the context's
 *   s2k_ctx_set_key_grouping hash_bits, one term pair per distinct key, the generator's term, the multiscalar core); it takes
 *   the whole batch only: lo == 0 and cnt == n.
 * form 1, the plain form: what the bisect calls run on a rejected batch - one term pair per item, the terms kept in the
 *   context's save area, then the sum over the sub-range [lo, lo + cnt) of the batch alone (coefficients by the item's index
 *   in the BATCH, not in the range), by the very functions the bisection runs.
 * out: the affine record 0x04 || X || Y of E, or 65 zero bytes for the identity.  *status: the device status word as read
 * back, non-zero when an item is out of the combination (an s, r or v out of range, an r or key that is no abscissa / point
 * of the curve).  It is the PREPARATION's word and the preparation runs over the whole batch: in form 1 it covers all n items,
 * not the sub-range (the sub-range step sets no status of its own).  in_comb (n bytes, or NULL): 1 for an item that took part
 * in the sum, 0 for one that was left out - after the key terms in form 0; all n items in form 1 as well.
 * S2K_ERR_ARG: a NULL pointer (msgs may be NULL when every message is empty), n == 0 or above 2^22, msg_len above 2^31 - 1, a
 * form other than 0 and 1, a range that is empty or not inside the batch, (ECDSA) flags other than S2K_ECDSA_REJECT_MALLEABLE.
 * Host pointers; synchronous; they use the context's staging buffer, its multiscalar workspace and its save area, so they are
 * not for use beside calls in flight. */
int s2k_debug_schnorr_rlc_point(s2k_ctx *ctx, size_t n, const uint8_t *pk /* n*32 */, const uint8_t *msgs,
                                const uint64_t *msg_offsets, size_t msg_len, const uint8_t *sig /* n*64 */,
                                const uint8_t *key32, int form, size_t lo, size_t cnt, uint8_t *out /* 65 */,
                                uint32_t *status, uint8_t *in_comb /* n or NULL */);
int s2k_debug_ecdsa_rlc_point(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy /* n*64 */, const uint8_t *digest32 /* n*32 */,
                              const uint8_t *r /* n*32 */, const uint8_t *s /* n*32 */, const uint8_t *recovery_id /* n */,
                              uint32_t flags, const uint8_t *key32, int form, size_t lo, size_t cnt, uint8_t *out /* 65 */,
                              uint32_t *status, uint8_t *in_comb /* n or NULL */);
/* Many independent sums in one call: out[j] = sum of k[i] * P[i] over i in [seg_offsets[j], seg_offsets[j+1]) — for every j
 * the record Point.MultiScalarMultVartime(scalars[a:b], points[a:b]) gives (point_mul_multi.go:73-117), so exactly what
 * s2k_multi_scalar_mult returns for that slice.  ONLY the Vartime form: variable time (data-dependent digit additions and
 * bucket sorts), public scalars only.  The constant-time Point.MultiScalarMult (:25-67) binds to s2k_ct_multi_scalar_mult
 * below, never to this.  seg_offsets is HOST memory in both forms (n_seg + 1 entries, seg_offsets[0] == 0, non-decreasing,
 * seg_offsets[n_seg] == n; anything else is S2K_ERR_ARG before any launch).  An empty segment gives the identity record
 * (65 zero bytes, :37); n_seg == 0 writes nothing.  Segments of at most S2K_MSM_SEG_CROSSOVER (16384) terms run Straus in
 * pieces of S2K_MSM_SEG_T (8) terms, one lane and one shared chain of doublings per piece, complete additions, all pieces of
 * all segments side by side; longer ones take the bucket method of s2k_multi_scalar_mult one after the other (one such
 * segment alone IS that call).  The two environment variables are read at every call: do not change them while another
 * thread is inside the library.  Workspace: 578 bytes per term on the Straus path and 108 per piece, a block of the context
 * allocated at the first call and kept until s2k_ctx_destroy (s2k_ctx_device_bytes counts no multiscalar workspace).  A malformed point record anywhere is
 * S2K_ERR_ARG for the call.  The device form takes device pointers and synchronises the stream once, at the end (it has
 * to read back the status word). */
int s2k_multi_scalar_mult_segments(s2k_ctx *ctx, size_t n, const uint8_t *k /* n*32 */, const uint8_t *points /* n*65 */,
                                   size_t n_seg, const uint64_t *seg_offsets /* n_seg+1 */, uint8_t *out /* n_seg*65 */);
int s2k_multi_scalar_mult_segments_device(s2k_ctx *ctx, size_t n, const void *d_k, const void *d_points,
                                          size_t n_seg, const uint64_t *seg_offsets /* host */, void *d_out /* n_seg*65 */,
                                          void *hip_stream);
/* The host-side plan of the segmented call as a pure function (no device, no context), for the tests.  piece_terms == 0 /
 * crossover == 0: the defaults the call uses (S2K_MSM_SEG_T, S2K_MSM_SEG_CROSSOVER).  summary: pieces, segments on the bucket
 * method, terms on the Straus path, workspace bytes the call reserves, longest bucket-method segment, piece_terms and
 * crossover used, runs of consecutive Straus terms (one front-end launch each).  The arrays may be NULL (counts only); else
 * piece i of the launch order (longest first) covers the terms [piece_first[i], piece_first[i] + piece_len[i]) and is
 * piece number piece_dest[i] in segment order; seg_desc[2j] is the first piece of segment j, seg_desc[2j+1] its piece
 * count, or 0x80000000 when it takes the bucket method.  Bad offsets or sizes: S2K_ERR_ARG, as the call. */
int s2k_debug_msm_segments_plan(size_t n, size_t n_seg, const uint64_t *seg_offsets, uint32_t piece_terms, uint64_t crossover,
                                uint64_t summary[8], size_t piece_cap, uint32_t *piece_first, uint32_t *piece_len,
                                uint32_t *piece_dest, uint32_t *seg_desc);

/* ---- point sets: fixed-base segmented sums from tables kept across calls -------------------
 * A caller that holds one []*Point across many MultiScalarMultVartime calls (vector commitments under one generator list,
 * coefficient sums over a fixed key list) pays the per-term table and all the doublings of s2k_multi_scalar_mult_segments
 * again in every call.  A POINT SET (the sibling of s2k_keyset; the reference's analogue is its precomputed generator table,
 * point_mul_table.go) holds, for a fixed list of m points, the true-affine multiples mag * 2^(c pos) * P_i for every digit
 * position pos of a c-bit signed recoding of a 128-bit half scalar and 1 <= mag <= 2^(c-1): a term of a sum is then
 * 2 * positions table additions and no doubling.  The set is an explicit object, not a cache: built once by the caller,
 * destroyed by the caller BEFORE its context, owned by the context that made it (it remembers the context's generation and
 * device; a set used with another context is S2K_ERR_ARG) and, like every object of a context, not locked.
 *   window_bits  4 or 8; 0 = automatic: 8 when m tables of that width take at most half of the device memory free at the
 *                time (capped by keyset_free_bytes of s2k_set_table_memory_budgets when that is set), else 4, and
 *                S2K_ERR_NOMEM when neither fits (an explicit width that does not fit: S2K_ERR_NOMEM as well).  The build
 *                needs half as much again as scratch, freed before the call returns.  Anything else, m == 0 or a null
 *                pointer: S2K_ERR_ARG before any launch.
 *   geometry     (s2k_pointset_geometry, a pure host function) out = {positions, entries per position, table bytes per point}:
 *                {33, 8, 16896} at 4 bits, {17, 128, 139264} at 8.  The layout is uniform: the last position, which only ever
 *                holds the recoding's carry digit (0 or 1), has all its entries too.
 *   records      0x04 || X || Y, canonical and on the curve, or the 65-byte identity record, exactly what the multiscalar
 *                calls accept.  A malformed record is S2K_ERR_ARG and no set is made.  An identity record is allowed, has no
 *                table and contributes nothing to any sum.
 * s2k_debug_pointset_entry copies entry (pos, mag) of point i to the host as X || Y (32 big-endian bytes each); for an
 * identity record it gives 64 zero bytes. */
typedef struct s2k_pointset s2k_pointset;
int s2k_pointset_create(s2k_ctx *ctx, size_t m, const uint8_t *points65 /* m*65, host */, int window_bits, s2k_pointset **out);
void s2k_pointset_destroy(s2k_pointset *ps);
size_t s2k_pointset_size(const s2k_pointset *ps);
int s2k_pointset_window_bits(const s2k_pointset *ps);
size_t s2k_pointset_device_bytes(const s2k_pointset *ps);
int s2k_pointset_geometry(int window_bits, uint64_t out[3]);
int s2k_debug_pointset_entry(const s2k_pointset *ps, size_t i, unsigned pos, unsigned mag, uint8_t out64[64]);
/* out[j] = sum of k[i] * P[point_index[i]] over i in [seg_offsets[j], seg_offsets[j+1]), P the points of the set: byte for
 * byte the record s2k_multi_scalar_mult_segments gives on the expanded point array, hence Point.MultiScalarMultVartime on
 * that slice (point_mul_multi.go:73-117).  ONLY the Vartime form: variable time (data-dependent table addresses and digit
 * additions), public scalars only; the constant-time Point.MultiScalarMult binds to s2k_ct_multi_scalar_mult, never to
 * this.  point_index == NULL is the dense shape: the term at position t of its segment uses point t (a segment longer
 * than the set is S2K_ERR_ARG before any launch).  An index >= m anywhere is S2K_ERR_ARG for the call.  Offsets, empty
 * segments, n_seg == 0, the term limit and the single synchronisation at the end are those of
 * s2k_multi_scalar_mult_segments.  Segments of at most S2K_POINTSET_CROSSOVER (16384) terms run in pieces of S2K_POINTSET_T
 * (8) terms, one lane per piece, complete additions only; longer ones are expanded from the set's records and take the
 * bucket method of s2k_multi_scalar_mult.  Both environment variables are read at every call: do not change them while
 * another thread is inside the library.  Workspace: the segmented call's block of the context (72 or 136 bytes per term
 * at 8- or 4-bit digits, 128 per piece). */
int s2k_pointset_multi_scalar_mult_segments(s2k_ctx *ctx, const s2k_pointset *ps, size_t n, const uint8_t *k /* n*32 */,
                                            const uint32_t *point_index /* n, or NULL */, size_t n_seg,
                                            const uint64_t *seg_offsets /* n_seg+1 */, uint8_t *out /* n_seg*65 */);
int s2k_pointset_multi_scalar_mult_segments_device(s2k_ctx *ctx, const s2k_pointset *ps, size_t n, const void *d_k,
                                                   const void *d_point_index /* n uint32, or NULL */, size_t n_seg,
                                                   const uint64_t *seg_offsets /* host */, void *d_out /* n_seg*65 */,
                                                   void *hip_stream);
/* The argument check of the two calls above as a pure function (no device, no context): m the size of the set, `indexed`
 * non-zero when a point_index array is given.  S2K_OK, or S2K_ERR_ARG as the call would answer before any launch. */
int s2k_debug_pointset_check_args(size_t m, size_t n, int indexed, size_t n_seg, const uint64_t *seg_offsets);
/* SEC1 decode of n fixed-size encodings (enc_len = 33: SetCompressedBytes point_s11n.go:140;
 * enc_len = 65: SetUncompressedBytes :178).  ok[i] = 1 and out[i] = point on success,
 * ok[i] = 0 and out[i] = zeros otherwise. */
int s2k_point_decode_batch(s2k_ctx *ctx, size_t n, size_t enc_len, const uint8_t *enc, uint8_t *out, uint8_t *ok);

/* ---- hashing to the curve (RFC 9380, secp256k1_XMD:SHA-256_SSWU_RO_ / _NU_; batched) --------
 * Public data, one independent item per message, VARIABLE TIME like everything on the GPU here.  The output is the 65-byte
 * point record the multiscalar entry points take (65 zero bytes for the identity).  Messages follow the convention of
 * s2k_schnorr_verify_batch: n strings of msg_len bytes each (msg_offsets == NULL), or concatenated with msg_offsets[n+1]
 * byte offsets (msg_offsets[0] == 0, non-decreasing; any lengths).  The domain separation tag is common to a call and is
 * HOST memory in every form.  Refused with S2K_ERR_ARG before any launch, the output untouched: a null context, a null
 * buffer with n > 0, n > 2^31 - 1, dst_len == 0 (h2c_expand_message.go:50-53), offsets that do not start at 0 or that
 * decrease.  n == 0 writes nothing and succeeds. */
#define S2K_H2C_SSWU_RO 0 /* hash_to_curve: two field elements, two mapped points, their sum */
#define S2K_H2C_SSWU_NU 1 /* encode_to_curve: one field element, one mapped point */
/* DST_prime of expand_message_xmd (h2c_expand_message.go:46-63,79-80): dst || I2OSP(dst_len, 1), and for a tag of more than
 * 255 bytes SHA-256("H2C-OVERSIZE-DST-" || dst) || 0x20.  Host function: no context, no device.  out holds up to 256 bytes;
 * *out_len receives the length.  dst_len == 0 (or a null pointer): S2K_ERR_ARG (:50-53). */
int s2k_h2c_dst_prime(const uint8_t *dst, size_t dst_len, uint8_t out[256], size_t *out_len);
/* out[i] = len_in_bytes uniform bytes for message i — expandMessageXMD with SHA-256 (h2c_expand_message.go:27-139).
 * len_in_bytes must be in 1..8160 (ell = ceil(len_in_bytes / 32) <= 255, :42-44,71-73). */
int s2k_expand_message_xmd_batch(s2k_ctx *ctx, size_t n, const uint8_t *dst, size_t dst_len, const uint8_t *msgs,
                                 const uint64_t *msg_offsets, size_t msg_len, size_t len_in_bytes,
                                 uint8_t *out /* n*len_in_bytes */);
/* out[i] = sum over j < count of Point.SetUniformBytes(uniform[(i*count + j)*len ...]) (point_h2c.go:23-55): the wide
 * reduction mod p (field.Element.SetWideBytes, internal/field/field_reduce.go:24-64; a 32-byte value >= p is reduced, not
 * refused), swu.MapToCurveSimpleSWU and swu.IsoMap (internal/swu/swu.go:70-199).  count is 1 or 2 — count = 2 is exactly
 * steps 2-5 of the RO suite (h2c.go:32-44) —, len in [32, 64]; anything else is S2K_ERR_ARG (the reference panics). */
int s2k_map_to_curve_batch(s2k_ctx *ctx, size_t n, size_t count, size_t len, const uint8_t *uniform /* n*count*len */,
                           uint8_t *out /* n*65 */);
/* out[i] = Secp256k1_XMD_SHA256_SSWU_RO(dst, msg_i) (suite S2K_H2C_SSWU_RO, h2c.go:25-45) or
 * Secp256k1_XMD_SHA256_SSWU_NU(dst, msg_i) (S2K_H2C_SSWU_NU, h2c.go:49-63), one kernel from message bytes to record. */
int s2k_hash_to_curve_batch(s2k_ctx *ctx, int suite, size_t n, const uint8_t *dst, size_t dst_len, const uint8_t *msgs,
                            const uint64_t *msg_offsets, size_t msg_len, uint8_t *out /* n*65 */);
/* The same on device pointers and the caller's stream (the tag stays host memory), chained behind the context's earlier
 * calls like the other *_device forms; it synchronises the stream once, at the end, to read back its status word.  The
 * offsets are device memory here, so the caller states the size of the message buffer: total_msg_bytes.  No lane reads
 * outside [0, total_msg_bytes): an item whose range is not inside it, or whose offsets decrease (or do not start at 0),
 * gets the identity record and the call returns S2K_ERR_ARG; the other records are written.  With msg_offsets == NULL,
 * n * msg_len > total_msg_bytes is refused before any launch. */
int s2k_hash_to_curve_batch_device(s2k_ctx *ctx, int suite, size_t n, const uint8_t *dst /* host */, size_t dst_len,
                                   const void *d_msgs, const void *d_msg_offsets, size_t msg_len, size_t total_msg_bytes,
                                   void *d_out /* n*65 */, void *hip_stream);

/* ---- constant-time twins, host CPU (no GPU, no context) ------------------------------------
 * What the reference's secret-handling code calls.  No branch, address or
 * loop count depends on the scalar, the private key or the nonce: masked full-table scans
 * (lookupProjectivePoint / lookupAffinePoint, point_mul_table_ref.go:11-24), arithmetic selects,
 * complete formulas.  Point arguments are public (the peer's key) and are validated like
 * SetUncompressedBytes (point_s11n.go:178); a malformed record is S2K_ERR_ARG. */
/* out = k*P — Point.ScalarMult (point_mul_glv.go:257-303); k is reduced mod n (SetBytes) */
int s2k_ct_scalar_mult(const uint8_t k[32], const uint8_t point65[65], uint8_t out65[65]);
/* out = sum_i k[i]*P[i] — Point.MultiScalarMult (point_mul_multi.go:25-67), the CONSTANT-TIME form: Straus with one
 * 15-entry table per point, masked full-table scans (projectivePointMultTable.SelectAndAdd, point_mul_table.go:34-41),
 * doublings shared by all terms; n == 1 is Point.ScalarMult (:31-33), n == 0 the identity.  The scalars (reduced mod n,
 * SetBytes) are secret; the points and n are public.  This — not s2k_multi_scalar_mult — is what Point.MultiScalarMult
 * binds to; only MultiScalarMultVartime (:73-117) may go to the GPU.  Cost: 15 n complete additions for the tables,
 * 252 doublings, 64 n additions; 1440 n bytes of scratch (S2K_ERR_NOMEM if it cannot be had, S2K_ERR_ARG for a
 * malformed record or n > 2^24). */
int s2k_ct_multi_scalar_mult(size_t n, const uint8_t *k /* n*32 */, const uint8_t *points65 /* n*65 */, uint8_t out65[65]);
/* out = k*G — Point.ScalarBaseMult (point_mul_table.go:168-194) */
int s2k_ct_scalar_base_mult(const uint8_t k[32], uint8_t out65[65]);
/* shared_x = x(d*Q) — PrivateKey.ECDH (secec/secec.go:53-56); d in [1,n), Q a valid public key */
int s2k_ct_ecdh(const uint8_t priv32[32], const uint8_t pub65[65], uint8_t shared_x[32]);
/* The arithmetic of PrivateKey.Sign (secec/ecdsa.go:335-390) for a caller-supplied nonce k:
 * r = x(k*G) mod n, s = (e + r*d)/k mod n normalised to s <= n/2, and the recovery id.  The nonce
 * derivation (ecdsa.go:284-333) stays in the caller.  S2K_ERR_ARG: d or k outside [1,n), or r == 0
 * or s == 0 (draw another nonce, as the reference does). */
int s2k_ct_ecdsa_sign_raw(const uint8_t priv32[32], const uint8_t digest32[32], const uint8_t nonce32[32],
                          uint8_t r32[32], uint8_t s32[32], uint8_t *recovery_id);
/* ---- single operations of Point / Scalar / field.Element: constant time, host CPU ----------------------------------
 * What the reference's Point / Scalar / field.Element METHODS bind to.  One call, one operation, no context, no
 * device: the batched GPU forms further down (s2k_point_add_batch, s2k_fn_op_batch, s2k_fp_op_batch) are variable time and
 * cost a device round trip - they are batch offerings for public data, never the binding of a method that may see a secret
 * (Scalar.Invert of a nonce, ecdsa.go:371).  No branch or address depends on an operand's VALUE, including whether a point is
 * the identity.  Points are 65-byte records, scalars / elements 32-byte canonical big-endian; an operand the reference's type
 * cannot hold (off-curve or non-canonical: its constructors return errors, point.go:192-216, scalar.go:135, field.go:153) is
 * S2K_ERR_ARG.  ctrl follows the reference: 0 selects the first alternative, anything else the second. */
int s2k_ct_point_add(const uint8_t a65[65], const uint8_t b65[65], uint8_t out65[65]);        /* Point.Add, point.go:62 */
int s2k_ct_point_double(const uint8_t a65[65], uint8_t out65[65]);                             /* Point.Double, point.go:73 */
int s2k_ct_point_subtract(const uint8_t a65[65], const uint8_t b65[65], uint8_t out65[65]);   /* Point.Subtract, point.go:83 */
int s2k_ct_point_negate(const uint8_t a65[65], uint8_t out65[65]);                             /* Point.Negate, point.go:89 */
int s2k_ct_point_conditional_negate(const uint8_t a65[65], uint64_t ctrl, uint8_t out65[65]); /* Point.ConditionalNegate, point.go:102 */
int s2k_ct_point_conditional_select(const uint8_t a65[65], const uint8_t b65[65], uint64_t ctrl,
                                    uint8_t out65[65]);                                        /* Point.ConditionalSelect, point.go:115 */
int s2k_ct_point_equal(const uint8_t a65[65], const uint8_t b65[65], uint64_t *out);          /* Point.Equal, point.go:133: 1 / 0 */
int s2k_ct_point_is_identity(const uint8_t a65[65], uint64_t *out);                            /* Point.IsIdentity, point.go:148 */
int s2k_ct_point_is_y_odd(const uint8_t a65[65], uint64_t *out);                               /* Point.IsYOdd, point.go:155 */
/* op: S2K_OP_MUL / SQR / ADD / SUB / NEG / INV (below) - Scalar.Multiply / Square / Add / Subtract / Negate (scalar.go:66-93),
 * Scalar.Invert (scalar_invert.go:11; 0 -> 0).  b32 is read by MUL / ADD / SUB only. */
int s2k_ct_scalar_op(int op, const uint8_t a32[32], const uint8_t b32[32], uint8_t out32[32]);
int s2k_ct_scalar_conditional_select(const uint8_t a32[32], const uint8_t b32[32], uint64_t ctrl, uint8_t out32[32]); /* scalar.go:176 */
int s2k_ct_scalar_conditional_negate(const uint8_t a32[32], uint64_t ctrl, uint8_t out32[32]);                        /* scalar.go:168 */
/* what: 0 Scalar.IsZero (scalar.go:187), 1 Scalar.IsGreaterThanHalfN (:196), 2 Scalar.Equal (:182, reads b32): *out = 1 / 0 */
#define S2K_SCALAR_IS_ZERO 0
#define S2K_SCALAR_IS_GT_HALF_N 1
#define S2K_SCALAR_EQUAL 2
int s2k_ct_scalar_predicate(int what, const uint8_t a32[32], const uint8_t b32[32], uint64_t *out);
/* Scalar.SetBytes (scalar.go:123): out = src mod n; *did_reduce (may be NULL) = 1 iff src >= n.  Accepts any 32 bytes. */
int s2k_ct_scalar_set_bytes(const uint8_t src32[32], uint8_t out32[32], uint64_t *did_reduce);
/* field.Element: S2K_OP_MUL / SQR / ADD / SUB / NEG (internal/field/field.go:61-104), S2K_OP_INV (field_invert.go:11; 0 -> 0),
 * S2K_OP_SQRT (field_sqrt_ratio.go:14: *flag = 1 iff a is a square, out = a^((p+1)/4) then, 0 otherwise; flag required). */
int s2k_ct_fe_op(int op, const uint8_t a32[32], const uint8_t b32[32], uint8_t out32[32], uint64_t *flag);
/* Test instrumentation: field multiplications executed by the calling thread in s2k_ct_* since the
 * previous call of this function.  The count is the same for every scalar (tests/test_ct_cpu.py). */
uint64_t s2k_ct_debug_fe_mul_count(void);

/* ---- field / scalar element operations (batched; host pointers) -------------------- */
/* Element / Scalar methods, for API parity and for the parity tests of the device
 * arithmetic.  Inputs are reduced first (SetBytes semantics, field.go:115, scalar.go:123). */
enum {
  S2K_OP_MUL = 0, /* Multiply (field.go:82, scalar.go:84) */
  S2K_OP_SQR = 1, /* Square */
  S2K_OP_ADD = 2, /* Add */
  S2K_OP_SUB = 3, /* Subtract */
  S2K_OP_NEG = 4, /* Negate */
  S2K_OP_INV = 5, /* Invert (field_invert.go:11, scalar_invert.go:11); 0 -> 0 */
  S2K_OP_SQRT = 6 /* Fp only: Sqrt (field_sqrt_ratio.go:14); flag[i] = root exists */
};
int s2k_fp_op_batch(s2k_ctx *ctx, int op, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *flag);
int s2k_fn_op_batch(s2k_ctx *ctx, int op, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out, uint8_t *flag);
/* GLV split (point_mul_glv.go:59): k == k1 + k2*lambda (mod n), both canonical */
int s2k_fn_split_glv_batch(s2k_ctx *ctx, size_t n, const uint8_t *k, uint8_t *k1, uint8_t *k2);

/* Test access to the arithmetic of the hot kernels (impl must be S2K_IMPL_FAST): the 9x29 lazy
 * field of the verification ladder incl. its fused products, the Jacobian doubling / mixed
 * addition (jacobian29.h) and the complete 9x29 formulas of the multiscalar kernels (pt29.h), on
 * operands put in LAZY form first (same value, unreduced limbs; `lazy` holds a 4-bit code per
 * operand: bits 1:0 = multiples of p added limb-wise, bit 2 = borrow-spread).  in[0..4] are
 * n*32-byte big-endian operands a..e (NULL = unused); results are canonical.  Reference symbols
 * served: fiat Mul/Square/Add/Opp (secp256k1montgomery.go:87,418,750,844), Element.Invert / Sqrt
 * (field_invert.go:11, field_sqrt_ratio.go:14), addMixed / addComplete / doubleComplete
 * (point_projective.go:123,24,208).
 *   MUL a*b | SQR a^2 | MUL_PLUS a*b+c | SQR_PLUS a^2+b | MUL_ADD_MUL a*b+c*d | MUL_ADD_SQR a*b+c^2
 *   ADD a+b | NEGATE -a | HALF a/2 | NORMALIZE a (flag = a == 0) | COND_NEGATE1 (b odd ? -a : a)
 *   INV | SQRT (flag = root exists) | EQ (flag) | MUL_SMALL21 21a | NORMALIZE_WEAK a
 *   JDBL: 2P, JADD: P + (d,e) for P = (a,b) lifted to Jacobian Z = c; out,out2 = affine x,y;
 *         flag = 0 when the incomplete formulas hit an exceptional case (Z3 = 0)
 *   PT29_DBL / PT29_ADD / PT29_ADD_MIXED: complete formulas, P = (a:b:1) scaled by Z = c
 *         (c = 0: the identity), Q = (d,e); flag = 0 when the result is the identity */
enum {
  S2K_HP_MUL = 0, S2K_HP_SQR, S2K_HP_MUL_PLUS, S2K_HP_SQR_PLUS, S2K_HP_MUL_ADD_MUL, S2K_HP_MUL_ADD_SQR,
  S2K_HP_ADD, S2K_HP_NEGATE, S2K_HP_HALF, S2K_HP_NORMALIZE, S2K_HP_COND_NEGATE1, S2K_HP_INV, S2K_HP_SQRT,
  S2K_HP_EQ, S2K_HP_MUL_SMALL21, S2K_HP_NORMALIZE_WEAK, S2K_HP_JDBL, S2K_HP_JADD, S2K_HP_PT29_DBL,
  S2K_HP_PT29_ADD, S2K_HP_PT29_ADD_MIXED,
  S2K_HP_INV_GCD,   /* fe29_inv_gcd: the safegcd inversion mod p of the per-key tables (same values as S2K_HP_INV) */
  S2K_HP_JADD_FULL, /* jpt29_add: P as for JADD, Q = (d, e) lifted to Z2 = c^2 */
  /* pt29q.h: the complete formulas spread over the four lanes of a quad (the serial tail of the multi-scalar
   * multiplication); inputs and outputs as PT29_DBL / PT29_ADD (Q scaled by c as well).  Bits 20.. of `lazy`: how often
   * the operation is chained on its own result (P + Q + Q + ..., 2^k P); 0 means once. */
  S2K_HP_PT29Q_DBL, S2K_HP_PT29Q_ADD,
  /* xyzz29_add_affine (xyzz29.h: the bucket pass's incomplete mixed addition): P = (a, b) lifted to ZZ = c^2, ZZZ = c^3,
   * Q = (d, e); flag = 0 when P and Q share their x (ZZ3 = 0: the piece is re-done with the complete formulas) */
  S2K_HP_XYZZ_ADD,
  /* one round border of the keyed ladder as k_verify_fast<ECDSA_KEYED> runs it: P lifted as for XYZZ_ADD, + Q in XYZZ,
   * XYZZ -> Jacobian, two Jacobian doublings, Jacobian -> XYZZ, + Q in XYZZ, XYZZ -> Jacobian: out = 4 P + 5 Q;
   * flag = 0 when Z ends as 0 (P = +-Q: ZZ = 0 must survive the changes of form and the doublings) */
  S2K_HP_XYZZ_ROUND,
  /* fe29r.h: the field with one limb per lane of a 16-lane DPP row, the complete formulas with one product per row (the
   * serial tail of the multi-scalar multiplication since round 5; ONE WAVE per item).  FER_MUL a*b, FER_MUL_PLUS a*b+c,
   * FER_MUL_ADD_MUL a*b+c*d, FER_SMALL 21a: the item's four rows multiply four different lazy forms of the operands, flag =
   * the rows agree.  PT29R_DBL / PT29R_ADD: inputs, outputs and chaining (bits 20.. of `lazy`) as PT29Q_*; bit 0 of `lazy`:
   * P's y with two units; flag 2 = the rows disagree.  FER_SWAPS (n >= 8): out[0..255] = the lane numbers after
   * v_permlane16_swap (even | odd rows) and v_permlane32_swap (low | high half). */
  S2K_HP_FER_MUL, S2K_HP_FER_MUL_PLUS, S2K_HP_FER_MUL_ADD_MUL, S2K_HP_FER_SMALL, S2K_HP_PT29R_DBL, S2K_HP_PT29R_ADD, S2K_HP_FER_SWAPS,
  /* arithmetic mod n.  sc26.h (the lazy 10 x 26 Montgomery form of the scalar preparation, R = 2^260; bit 0 of an operand's
   * code in `lazy` adds n to it): SC26_MUL a*b/R | SC26_SQR a^2/R | SC26_TO_MONT a*R | SC26_TO_SC a (a < 2n) | SC26_INV
   * a^-1 R^2 (Montgomery inverse, a < 2n, 0 -> 0) | SC26_CHAIN acc = a, acc = acc*b/R as often as bits 20.. of `lazy` say (0: once).  out =
   * the raw lazy result mod 2^256, flag bit 0 = its bit 256, flag bit 1 = its limbs are in bounds, out2 = it reduced mod n.
   * sc.h (8 x 32, canonical operands taken as they are): SC_MONTMUL a*b/2^256 | SC_TO_MONT a*2^256 | SC_MONT_INV (the
   * Fermat chain) | SC_ADD a+b | SC_NEG -a | SC_REDUCE_ONCE (a < 2n) | SC_GT_HALF_N (flag = a > (n-1)/2) */
  S2K_HP_SC26_MUL, S2K_HP_SC26_SQR, S2K_HP_SC26_TO_MONT, S2K_HP_SC26_TO_SC, S2K_HP_SC26_INV, S2K_HP_SC26_CHAIN,
  S2K_HP_SC_MONTMUL, S2K_HP_SC_TO_MONT, S2K_HP_SC_MONT_INV, S2K_HP_SC_ADD, S2K_HP_SC_NEG, S2K_HP_SC_REDUCE_ONCE,
  S2K_HP_SC_GT_HALF_N,
  /* aff29.h, the affine formulas of the wide joint tables (one safegcd inversion each; no curve constant, so any curve
   * y^2 = x^3 + b): AFF_DBL (a, b) -> 2 (a, b) | AFF_ADD (a, b) + (c, d), x1 != x2.  Operands in their lazy forms; bits 20..
   * of `lazy` chain the operation on its own result (2^k P; P + k Q), 0 means once; out, out2 = x, y canonical. */
  S2K_HP_AFF_DBL, S2K_HP_AFF_ADD,
  /* xyzz29_add_affine_first (xyzz29.h: the first addition of k_generator_part, both points affine): P = (a, b), Q = (d, e) in
   * their lazy forms; out, out2 as XYZZ_ADD; flag = 0 when P and Q share their x (ZZ3 = ZZZ3 = 0) */
  S2K_HP_XYZZ_ADD_FIRST,
  /* fe29r.h, pt29r_add_b3: the complete addition on y^2 = x^3 + 7 c^6, the curve a key set's table entries live on (operand
   * c is W, non-zero; b3 = 21 c^6 is a field element there, not a small constant).  P = (a, b) and Q = (d, e) are points of
   * secp256k1 given affine ((0, 0): the identity), moved to that curve by (x c^2, y c^3) on the device, added there and
   * moved back: out, out2, flag, bit 0 of `lazy` and chaining (P + k Q) as PT29R_ADD. */
  S2K_HP_PT29R_ADD_B3,
  /* the comb ladder's column (jacobian29.h: coz29_pair_sum, jpt29_rescale, jpt29_add_affine), through s2k_fp_op_batch_ex8
   * only - it takes more operands than s2k_fp_op_batch_ex has slots: acc + s1 E1 + s2 E2 for acc = (in[0], in[1]) lifted to
   * Jacobian Z = in[2] as for JADD (bit 3 of in[2]'s lazy code: no lift; in[2] = 0: Z = 0), E1 = (in[3], in[4]) and E2 =
   * (in[5], in[6]) affine with x1 != x2, in their lazy forms (one unit each), s1 = -1 when bit 0 of in[7] is set, s2 = -1 when
   * its bit 1 is (in[7] NULL: both +1).  out, out2 = affine x, y; flag = 0 when Z3 = 0 (E1 = +-E2, acc = +-(s1 E1 + s2 E2),
   * Z = 0).  reps == 0: once; reps >= 1: `reps` times the column with one jpt29_double behind it, as the ladder runs them. */
  S2K_HP_JADD_PAIR,
  /* a round of the wave-per-signature comb ladder (small_call.hip: row_ladder_comb), through s2k_fp_op_batch_ex with the operands
   * of PT29R_ADD_B3: Q = (d, e) is moved to y^2 = x^3 + 7 c^6 as there and comes back as the projective point (x c : y : c^3)
   * of secp256k1 (fe29r.h: pt29r_pair_from_iso, both halves of the layer in turn); the accumulator starts at P = (a, b) and
   * each repetition is acc = pt29r_add(pt29r_double(acc), Q): 2^reps P + (2^reps - 1) Q.  out, out2, flag, bit 0 of `lazy`
   * and the repetition count as PT29R_ADD. */
  S2K_HP_PT29R_COMB_STEP
};
int s2k_fp_op_batch_ex(s2k_ctx *ctx, uint32_t impl, int op, uint32_t lazy, size_t n, const uint8_t *const in[5],
                       uint8_t *out, uint8_t *out2, uint8_t *flag);
/* the same for operations of up to eight operands (S2K_HP_JADD_PAIR): `lazy` holds the 4-bit code of in[j] in bits
 * 4j .. 4j + 3, so the chaining count has an argument of its own */
int s2k_fp_op_batch_ex8(s2k_ctx *ctx, uint32_t impl, int op, uint32_t lazy, uint32_t reps, size_t n,
                        const uint8_t *const in[8], uint8_t *out, uint8_t *out2, uint8_t *flag);
/* The odd GLV split the verification ladder uses (sc_split_glv_odd): k == (-1)^s1 k1 + (-1)^s2 k2 lambda
 * (mod n) with k1, k2 ODD and below 2^129 (32-byte big-endian magnitudes), signs[i] = s1 | s2 << 1.
 * Serves splitGLV (point_mul_glv.go:59); impl must be S2K_IMPL_FAST. */
int s2k_fn_split_glv_batch_ex(s2k_ctx *ctx, uint32_t impl, size_t n, const uint8_t *k, uint8_t *k1, uint8_t *k2,
                              uint8_t *signs);

/* ---- SHA-2 and Keccak message digests on the device, and ECDSA verification from messages -------- */
/* The reference's ECDSA callers start from a message and a hash: h := sha256.Sum256(m); pk.Verify(h[:], sig, opts).  The
 * calls above take h; these take m and hash on the device (one lane per message), so no per-item work is left on the host.
 *   S2K_HASH_SHA256   SHA-256(m)
 *   S2K_HASH_SHA256D  SHA-256(SHA-256(m)), Bitcoin's message hash: one more compression
 *   S2K_HASH_SHA512   SHA-512(m); a verification call uses its leftmost 32 bytes, which is what the reference's hashToScalar
 *                     does with a hash longer than the order (secec/ecdsa.go:477-486)
 *   S2K_HASH_KECCAK256  Keccak-256(m) as submitted (padding 0x01 .. 0x80): Ethereum's message and address hash
 *   S2K_HASH_SHA3_256   SHA3-256(m) of FIPS 202: the same permutation and rate (136 bytes), domain byte 0x06
 * The two Keccak ids run in a kernel of their own (k_digest_keccak); out_len is 32 for them.
 * Messages follow the convention of s2k_schnorr_verify_batch: n strings of msg_len bytes each (msg_offsets == NULL), or one
 * blob with msg_offsets[n + 1] byte offsets (any lengths, zero included; msg_offsets[0] need not be 0).  Every message is
 * shorter than 2^31 bytes.
 *
 * s2k_digest_batch: out[i * out_len .. + out_len) = the digest of message i.  out_len is 32 - the whole SHA-256 / SHA-256d
 * digest, or the leftmost 32 bytes of SHA-512 - or 64 with S2K_HASH_SHA512, the whole digest.  This is the digest the
 * verification calls take: the encoded, whole-batch and group calls have no messages form of their own and are
 * reached as s2k_digest_batch_device followed by the existing call on the same stream, without a host round trip (recovery
 * has one where it returns addresses: s2k_ecdsa_recover_address_messages_batch below).
 * _device: device pointers, chained on the caller's stream like the other *_device forms; does not synchronise.
 *
 * s2k_ecdsa_verify_messages_batch[_device/_submit], ..._keyset[_device], ..._keyset_bykey[_device]: the arguments of
 * s2k_ecdsa_verify_batch[...] and its key-set forms with digest32 replaced by (alg, msgs, msg_offsets, msg_len).  Each runs
 * the digest kernel into a buffer of the context (32 bytes per item, allocated on the first such call and kept), then the
 * unchanged path of its digest sibling on the same stream: valid[i] is bit for bit what the sibling gives on the digests of
 * the messages, on every ladder its dispatch picks, and s2k_ctx_key_grouping_stats / s2k_ctx_last_keyset_ladder read as
 * after the sibling.  _submit: messages, offsets, keys and signatures must stay alive until s2k_wait, like the other inputs.
 *
 * S2K_ERR_ARG before anything is launched, outputs untouched, for every form: an unknown alg, a NULL buffer with n > 0,
 * msg_len >= 2^31, an out_len other than the above, n >= 2^30, and whatever the digest sibling refuses (a key set of another
 * context, S2K_ECDSA_FORCE_COMPLETE over a key set, ...).  n == 0 succeeds and writes nothing.
 * The HOST forms scan the offsets and refuse, the same way, offsets that decrease and items of 2^31 bytes or more.
 * PRECONDITION of the _device forms, as for s2k_schnorr_verify_batch_device: the offsets on the device never decrease, every
 * item is shorter than 2^31 bytes and msg_offsets[n] is within the blob.  They cannot check this without a round trip and do
 * not: a decreasing offset makes the device read outside the blob.
 *
 * Cost: lanes of a wavefront with different block counts run to the longest of them, so a batch with one very long message
 * is slow, not wrong; there is no second kernel for it.  Out of scope here: messages forms of the encoded,
 * whole-batch and group calls (see above), SHA3-512 and SHAKE, Keccak for the BIP-340 or whole-batch calls, tagged hashes
 * (BIP-340's challenge is computed by the Schnorr calls), and a cooperative kernel for single huge messages.
 * s2k_ctx_device_bytes does not count the 32 n bytes of the digest buffer.
 *
 * Test hooks.  s2k_debug_digest_caps: out[0] = the bytes of LDS a workgroup stages the stretch of its 256 messages in; a
 * stretch at addresses [lo, hi) is staged when (hi - (lo & ~15)) + 16 <= that capacity, else read in place.
 * s2k_debug_digest_strided: s2k_digest_batch with rows out_stride (out_len .. 4096) bytes apart; out[n * out_stride] goes to
 * the device as the caller filled it and comes back whole, so the bytes between the rows show that they were not written. */
#define S2K_HASH_SHA256 0
#define S2K_HASH_SHA256D 1
#define S2K_HASH_SHA512 2
#define S2K_HASH_KECCAK256 3   /* Keccak-256, original padding (0x01 .. 0x80), rate 136 */
#define S2K_HASH_SHA3_256  4   /* FIPS 202 SHA3-256: same permutation and rate, domain byte 0x06 */
int s2k_digest_batch(s2k_ctx *ctx, int alg, size_t n, const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                     uint8_t *out /* n*out_len */, size_t out_len);
int s2k_digest_batch_device(s2k_ctx *ctx, int alg, size_t n, const void *d_msgs, const void *d_msg_offsets, size_t msg_len,
                            void *d_out, size_t out_len, void *hip_stream);
int s2k_ecdsa_verify_messages_batch(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy /* n*64 */, int alg, const uint8_t *msgs,
                                    const uint64_t *msg_offsets, size_t msg_len, const uint8_t *r /* n*32 */,
                                    const uint8_t *s /* n*32 */, uint32_t flags, uint8_t *valid /* n */);
int s2k_ecdsa_verify_messages_batch_device(s2k_ctx *ctx, size_t n, const void *d_pub_xy, int alg, const void *d_msgs,
                                           const void *d_msg_offsets, size_t msg_len, const void *d_r, const void *d_s,
                                           uint32_t flags, void *d_valid, void *hip_stream);
int s2k_ecdsa_verify_messages_batch_submit(s2k_ctx *ctx, size_t n, const uint8_t *pub_xy, int alg, const uint8_t *msgs,
                                           const uint64_t *msg_offsets, size_t msg_len, const uint8_t *r, const uint8_t *s,
                                           uint32_t flags, uint8_t *valid, s2k_ticket *ticket);
int s2k_ecdsa_verify_messages_batch_keyset(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint32_t *key_index /* n */,
                                           int alg, const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                                           const uint8_t *r, const uint8_t *s, uint32_t flags, uint8_t *valid);
int s2k_ecdsa_verify_messages_batch_keyset_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_key_index,
                                                  int alg, const void *d_msgs, const void *d_msg_offsets, size_t msg_len,
                                                  const void *d_r, const void *d_s, uint32_t flags, void *d_valid,
                                                  void *hip_stream);
int s2k_ecdsa_verify_messages_batch_keyset_bykey(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const uint8_t *pub_xy, int alg,
                                                 const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                                                 const uint8_t *r, const uint8_t *s, uint32_t flags, uint8_t *valid);
int s2k_ecdsa_verify_messages_batch_keyset_bykey_device(s2k_ctx *ctx, const s2k_keyset *ks, size_t n, const void *d_pub_xy,
                                                        int alg, const void *d_msgs, const void *d_msg_offsets, size_t msg_len,
                                                        const void *d_r, const void *d_s, uint32_t flags, void *d_valid,
                                                        void *hip_stream);
int s2k_debug_digest_caps(uint32_t out[1]);
int s2k_debug_digest_strided(s2k_ctx *ctx, int alg, size_t n, const uint8_t *msgs, const uint64_t *msg_offsets, size_t msg_len,
                             uint8_t *out /* n*out_stride */, size_t out_len, size_t out_stride);

/* ---- Keccak-256 addresses: of key records, and of the keys recovered from signatures -------- */
/* Callers who recover keys in bulk want the 20-byte address Keccak-256(X || Y)[12..32), and started from a message whose
 * digest is Keccak-256 too.  These calls leave neither hash on the host and move 20 bytes per item back instead of 65.
 *
 * s2k_keccak_address_batch[_device]: addr20[i] = Keccak-256(pub65[i][1..65))[12..32) when pub65[i][0] == 0x04 and (ok == NULL or
 * ok[i] != 0); else 20 zero bytes.  The record is hashed as given: no curve check (these are records this library produced,
 * or keys the caller vouches for).  One kernel, k_keccak_address, one lane per record; records and rows may lie at any
 * alignment, exactly 20 n bytes are written.
 *
 * s2k_ecdsa_recover_address_batch[_device]: s2k_ecdsa_recover_batch, then the address of each recovered key: ok[i] is bit for
 * bit that call's ok[i], addr20[i] the address of its pub65[i], 20 zero bytes where ok[i] == 0.  flags as
 * s2k_ecdsa_recover_batch.  The recovery runs unchanged, on whatever ladder its dispatch picks, into a buffer of the context
 * (65 bytes per item, allocated on the first such call and kept; s2k_ctx_device_bytes does not count it), and
 * k_keccak_address runs behind it on the same stream: one launch more than the plain recovery.
 *
 * s2k_ecdsa_recover_address_messages_batch[_device]: the same with digest32 replaced by (alg, msgs, msg_offsets, msg_len),
 * conventions of s2k_digest_batch, any S2K_HASH_* id; the digest kernel runs in front, into the context's digest buffer.
 *
 * S2K_ERR_ARG before anything is launched, outputs untouched: a NULL ctx, a NULL buffer with n > 0 (the ok of
 * s2k_keccak_address_batch[_device] may be NULL), n >= 2^30, an unknown alg, msg_len >= 2^31, and on the host forms offsets
 * that decrease or items of 2^31 bytes or more.  n == 0 succeeds and writes nothing.  The _device forms carry the digest
 * calls' PRECONDITION on the offsets.
 *
 * Out of scope here: a match form (valid[i] = recovered address == expected), ticket (_submit) forms of the recovery calls,
 * Keccak for the BIP-340 or whole-batch calls, SHA3-512 / SHAKE, RIPEMD-160 addresses, and fusing the hash into the kernels
 * that write key records. */
int s2k_keccak_address_batch(s2k_ctx *ctx, size_t n, const uint8_t *pub65 /* n*65 */, const uint8_t *ok /* n, or NULL */,
                             uint8_t *addr20 /* n*20 */);
int s2k_keccak_address_batch_device(s2k_ctx *ctx, size_t n, const void *d_pub65, const void *d_ok, void *d_addr20,
                                    void *hip_stream);
int s2k_ecdsa_recover_address_batch(s2k_ctx *ctx, size_t n, const uint8_t *digest32 /* n*32 */, const uint8_t *r /* n*32 */,
                                    const uint8_t *s /* n*32 */, const uint8_t *recovery_id /* n */, uint32_t flags,
                                    uint8_t *addr20 /* n*20 */, uint8_t *ok /* n */);
int s2k_ecdsa_recover_address_batch_device(s2k_ctx *ctx, size_t n, const void *d_digest32, const void *d_r, const void *d_s,
                                           const void *d_recovery_id, uint32_t flags, void *d_addr20, void *d_ok,
                                           void *hip_stream);
int s2k_ecdsa_recover_address_messages_batch(s2k_ctx *ctx, size_t n, int alg, const uint8_t *msgs, const uint64_t *msg_offsets,
                                             size_t msg_len, const uint8_t *r, const uint8_t *s, const uint8_t *recovery_id,
                                             uint32_t flags, uint8_t *addr20, uint8_t *ok);
int s2k_ecdsa_recover_address_messages_batch_device(s2k_ctx *ctx, size_t n, int alg, const void *d_msgs,
                                                    const void *d_msg_offsets, size_t msg_len, const void *d_r, const void *d_s,
                                                    const void *d_recovery_id, uint32_t flags, void *d_addr20, void *d_ok,
                                                    void *hip_stream);

/* ---- introspection used by the tests ------------------------------------------------ */
/* Copies generator-table entry T_i[d] (X‖Y big-endian) to out64.  Layout: DESIGN.md §3. */
/* window width (bits) the automatic generator tables of this library aim for (a build-time constant: S2K_GT_BITS); what a
 * context uses at a given moment: s2k_ctx_gt_info.  s2k_debug_gtable_entry reads the table the context uses now. */
int s2k_generator_window_bits(void);
int s2k_debug_gtable_entry(s2k_ctx *ctx, unsigned i, unsigned d, uint8_t *out64);

#ifdef __cplusplus
}
#endif
#endif
