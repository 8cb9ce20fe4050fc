"""secp256k1_voi_amd — MI355X (gfx950) batch engine for the verify / scalar-mult path of
Yawning/secp256k1-voi.

This module is the thin Python binding of the C-ABI in include/secp256k1_voi_amd.h
(ctypes; no torch types cross the boundary).  All compute happens in the HIP library
``libsecp256k1_voi_amd.so`` built from csrc/; there is NO CPU fallback: importing works
everywhere, but creating an :class:`Engine` raises if the library or a GPU is missing.

Encodings are the reference's canonical ones: 32-byte big-endian scalars / coordinates,
65-byte point records (0x04‖X‖Y, or 65 zero bytes for the identity).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

# More than four HIP streams in a process (this engine holds up to four; torch and RCCL bring theirs) share the
# runtime's four default hardware queues and then run one after the other where the engine means them to overlap
# (measured: +0.28 ms on a 5.0 ms step once a process group exists).  The runtime reads this when
# it initialises, i.e. at the first HIP call of the process: importing this package before that is enough.
if "GPU_MAX_HW_QUEUES" not in os.environ:
    os.environ["GPU_MAX_HW_QUEUES"] = "8"      # (process-wide: export your own value to overrule it)
    import sys as _sys
    _t = _sys.modules.get("torch")
    if _t is not None and getattr(_t, "cuda", None) is not None and _t.cuda.is_initialized():
        import warnings
        warnings.warn("secp256k1_voi_amd: the HIP runtime was initialised before this package was imported, so "
                      "GPU_MAX_HW_QUEUES=8 comes too late; streams of the engine may share hardware queues "
                      "(export GPU_MAX_HW_QUEUES=8 in the environment instead)", RuntimeWarning)

_HERE = os.path.dirname(os.path.abspath(__file__))
# S2K_LIB: load another build of the library (a compile-time variant made with build(variant=...)), for
# same-box A/B runs that must not spend GPU time compiling
LIB_PATH = os.environ.get("S2K_LIB") or os.path.join(_HERE, "libsecp256k1_voi_amd.so")
CSRC = os.path.join(_HERE, "csrc")

REJECT_MALLEABLE = 1
BIP0066 = 2
FORCE_COMPLETE = 0x80000000
FORCE_WORKLIST = 0x40000000
ENCODING_ASN1, ENCODING_COMPACT, ENCODING_COMPACT_RECOVERABLE = 0, 1, 2
HASH_SHA256, HASH_SHA256D, HASH_SHA512 = 0, 1, 2    # S2K_HASH_*: the digest of the calls that take messages
HASH_KECCAK256, HASH_SHA3_256 = 3, 4                # ... Keccak-256 (original padding) and FIPS 202 SHA3-256

OP_MUL, OP_SQR, OP_ADD, OP_SUB, OP_NEG, OP_INV, OP_SQRT = range(7)
IMPL_COMPLETE, IMPL_FAST = 0, 1
CTX_WAIT_TABLES = 1
KEYS_OFF, KEYS_AUTO, KEYS_ALWAYS, KEYS_ADAPTIVE = 0, 1, 2, 3     # s2k_ctx_set_key_grouping (a new context: KEYS_ADAPTIVE)
LADDER_COMB, LADDER_WINDOW = 0, 1                                # s2k_ctx_set_keyed_ladder (a new context: LADDER_COMB)
KEYSET_AUTO, KEYSET_CHUNKS, KEYSET_JOINT, KEYSET_JOINT5, KEYSET_JOINT6, KEYSET_COMB = 0, 1, 2, 3, 4, 5   # s2k_keyset_create_ex
(HP_MUL, HP_SQR, HP_MUL_PLUS, HP_SQR_PLUS, HP_MUL_ADD_MUL, HP_MUL_ADD_SQR, HP_ADD, HP_NEGATE, HP_HALF, HP_NORMALIZE,
 HP_COND_NEGATE1, HP_INV, HP_SQRT, HP_EQ, HP_MUL_SMALL21, HP_NORMALIZE_WEAK, HP_JDBL, HP_JADD, HP_PT29_DBL, HP_PT29_ADD,
 HP_PT29_ADD_MIXED, HP_INV_GCD, HP_JADD_FULL, HP_PT29Q_DBL, HP_PT29Q_ADD, HP_XYZZ_ADD, HP_XYZZ_ROUND,
 HP_FER_MUL, HP_FER_MUL_PLUS, HP_FER_MUL_ADD_MUL, HP_FER_SMALL, HP_PT29R_DBL, HP_PT29R_ADD, HP_FER_SWAPS,
 HP_SC26_MUL, HP_SC26_SQR, HP_SC26_TO_MONT, HP_SC26_TO_SC, HP_SC26_INV, HP_SC26_CHAIN,
 HP_SC_MONTMUL, HP_SC_TO_MONT, HP_SC_MONT_INV, HP_SC_ADD, HP_SC_NEG, HP_SC_REDUCE_ONCE, HP_SC_GT_HALF_N,
 HP_AFF_DBL, HP_AFF_ADD, HP_XYZZ_ADD_FIRST, HP_PT29R_ADD_B3, HP_JADD_PAIR, HP_PT29R_COMB_STEP) = range(53)
KEYSET_LADDER_LANE, KEYSET_LADDER_ROW, KEYSET_LADDER_ROW_COMB = 0, 1, 2                  # s2k_ctx_last_keyset_ladder
H2C_SSWU_RO, H2C_SSWU_NU = 0, 1        # s2k_hash_to_curve_batch: hash_to_curve (random oracle) / encode_to_curve (non-uniform)

IDENTITY = bytes(65)


def pinned_array(shape, dtype=np.uint8) -> np.ndarray:
    """A numpy array in page-locked host memory (s2k_host_alloc): host-buffer calls copy from it asynchronously.
    The memory is released when the array (and every view of it) is gone."""
    import weakref
    lib = load_library()
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = lib.s2k_host_alloc(max(nbytes, 1))
    if not p:
        raise EngineError("s2k_host_alloc failed")
    buf = (C.c_uint8 * max(nbytes, 1)).from_address(p)
    weakref.finalize(buf, lib.s2k_host_free, p)
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def page_aligned_array(shape, dtype=np.uint8) -> np.ndarray:
    """A numpy array that owns whole pages (anonymous mmap, length rounded up to the page size): the kind of buffer to
    hand to host_register.  Registering a piece of the C heap pins and later unmaps pages that the allocator goes on
    using for other blocks (see s2k_host_register in the header)."""
    import mmap
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    page = mmap.PAGESIZE
    m = mmap.mmap(-1, max((nbytes + page - 1) // page * page, page))
    return np.frombuffer(m, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def host_register(a: np.ndarray) -> None:
    """Pin an existing (contiguous) array for asynchronous copies (s2k_host_register); undo with host_unregister
    before the array is released.  The array must own whole pages (page_aligned_array); a heap array is refused."""
    import mmap
    lib = load_library()
    nbytes, base = a.nbytes, a
    while getattr(base, "base", None) is not None:
        base = base.base
    if isinstance(base, memoryview):
        base = base.obj
    if isinstance(base, mmap.mmap) and a.ctypes.data % mmap.PAGESIZE == 0:
        nbytes = (nbytes + mmap.PAGESIZE - 1) // mmap.PAGESIZE * mmap.PAGESIZE   # the mapping owns the rest of its last page
    if lib.s2k_host_register(a.ctypes.data, nbytes) != 0:
        raise EngineError(lib.s2k_last_error(None).decode())


def host_unregister(a: np.ndarray) -> None:
    lib = load_library()
    if lib.s2k_host_unregister(a.ctypes.data) != 0:
        raise EngineError(lib.s2k_last_error(None).decode())


class EngineError(RuntimeError):
    pass


def build_variant(name: str, extra_flags: str, verbose: bool = False) -> str:
    """Build libsecp256k1_voi_amd.<name>.so with `extra_flags` next to the default library (own object
    directory); select it at run time with S2K_LIB=<path>."""
    from concurrent.futures import ThreadPoolExecutor
    units = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp"))]
    objdir = os.path.join(_HERE, "build", "variant_" + name)
    os.makedirs(objdir, exist_ok=True)
    out = os.path.join(_HERE, f"libsecp256k1_voi_amd.{name}.so")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", '-DS2K_BUILD_FLAGS="%s"' % extra_flags.replace('"', "'")]
    flags += extra_flags.split()

    def compile_one(u):
        obj = os.path.join(objdir, os.path.splitext(u)[0] + ".o")
        subprocess.check_call(["hipcc", *flags, "-c", os.path.join(CSRC, u), "-o", obj])
        return obj

    with ThreadPoolExecutor(max_workers=min(4, len(units))) as ex:
        objs = list(ex.map(compile_one, units))
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", out])
    if verbose:
        print("built", out)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP library for gfx950 with hipcc (cross-compiles without a GPU): one object
    per translation unit (in parallel), then one shared library.  The variant flags
    (S2K_EXTRA_FLAGS, e.g. "-DS2K_GT_BITS=16") are recorded next to the objects and compiled into
    s2k_build_config(); a library built with other flags than the ones asked for now is rebuilt,
    so an A/B script cannot leave a non-default kernel behind unnoticed."""
    from concurrent.futures import ThreadPoolExecutor
    units = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp"))]
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp"))]
    deps.append(os.path.join(os.path.dirname(_HERE), "include", "secp256k1_voi_amd.h"))
    if os.environ.get("S2K_LIB"):      # a prebuilt variant was selected: nothing to build
        return LIB_PATH
    objdir = os.path.join(_HERE, "build")
    stamp = os.path.join(objdir, "flags.stamp")
    extra = " ".join(os.environ.get("S2K_EXTRA_FLAGS", "").split())
    try:
        with open(stamp) as f:
            built_with = f.read()
    except OSError:
        built_with = None
    fresh = os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in deps)
    if not force and fresh and (built_with == extra or (built_with is None and not extra and not os.path.isdir(objdir))):
        return LIB_PATH
    os.makedirs(objdir, exist_ok=True)
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", '-DS2K_BUILD_FLAGS="%s"' % extra.replace('"', "'")]
    flags += extra.split()
    # the stamp names the flags of the objects in the directory: it is withdrawn while they are being replaced, so that an
    # interrupted build (a variant build, say) cannot leave objects of other flags under a stamp that vouches for them
    if not (built_with == extra):
        force = True
    try:
        os.remove(stamp)
    except OSError:
        pass

    # an object is reused when it is newer than its own source and every header, and was built with these flags
    headers = [d for d in deps if d.endswith(".h")]
    newest_header = max(os.path.getmtime(h) for h in headers)
    same_flags = built_with == extra and built_with is not None

    def compile_one(u):
        obj = os.path.join(objdir, os.path.splitext(u)[0] + ".o")
        src = os.path.join(CSRC, u)
        if not force and same_flags and os.path.exists(obj) and os.path.getmtime(obj) >= max(newest_header, os.path.getmtime(src)):
            return obj
        cmd = ["hipcc", *flags, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        return obj

    with ThreadPoolExecutor(max_workers=min(4, len(units))) as ex:
        objs = list(ex.map(compile_one, units))
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(extra)
    return LIB_PATH


_lib = None


def load_library() -> C.CDLL:
    """dlopen the engine.  Raises EngineError (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    vp, sz, u32, ci = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    lib.s2k_ctx_create.argtypes = [ci, C.POINTER(vp)]
    lib.s2k_ctx_destroy.argtypes = [vp]
    lib.s2k_ctx_destroy.restype = None
    lib.s2k_last_error.argtypes = [vp]
    lib.s2k_last_error.restype = C.c_char_p
    lib.s2k_version.restype = C.c_char_p
    lib.s2k_build_config.restype = C.c_char_p
    lib.s2k_ctx_profile.argtypes = [vp, ci]
    lib.s2k_ctx_profile_read.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.s2k_ctx_profile_read_stages.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.s2k_ctx_profile_msm.argtypes = [vp, ci]
    lib.s2k_ctx_profile_read_msm.argtypes = [vp, vp, vp]
    lib.s2k_ctx_set_key_grouping.argtypes = [vp, ci, u32, u32, u32]
    lib.s2k_ctx_set_keyed_ladder.argtypes = [vp, ci]
    lib.s2k_ctx_last_keyed_ladder.argtypes = [vp]
    lib.s2k_ctx_key_grouping_stats.argtypes = [vp, vp]
    lib.s2k_ctx_key_grouping_adaptive.argtypes = [vp, vp, ci]
    lib.s2k_ecdsa_verify_batch.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp]
    lib.s2k_ecdsa_verify_batch_device.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_recover_batch.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_recover_batch_device.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.s2k_ecdsa_batch_verify_rlc.argtypes = [vp, sz, vp, vp, vp, vp, vp, u32, vp, C.POINTER(ci)]
    lib.s2k_ecdsa_batch_verify_rlc_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, u32, vp, C.POINTER(ci), vp]
    lib.s2k_ecdsa_verify_recoverable_batch_bisect.argtypes = [vp, sz, vp, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.s2k_ecdsa_verify_recoverable_batch_bisect_device.argtypes = [vp, sz, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]
    lib.s2k_pack_valid_device.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.s2k_keyset_create.argtypes = [vp, sz, vp, C.POINTER(vp)]
    lib.s2k_keyset_create_ex.argtypes = [vp, sz, vp, ci, C.POINTER(vp)]
    lib.s2k_keyset_create_cap.argtypes = [vp, sz, vp, ci, sz, C.POINTER(vp)]
    lib.s2k_keyset_capacity.argtypes = [vp]
    lib.s2k_keyset_capacity.restype = sz
    lib.s2k_keyset_reserve.argtypes = [vp, sz]
    lib.s2k_keyset_append.argtypes = [vp, sz, vp, C.POINTER(u32)]
    lib.s2k_keyset_append_device.argtypes = [vp, sz, vp, C.POINTER(u32)]
    lib.s2k_keyset_replace.argtypes = [vp, sz, vp, vp]
    lib.s2k_keyset_replace_device.argtypes = [vp, sz, vp, vp]
    lib.s2k_keyset_remove.argtypes = [vp, sz, vp]
    lib.s2k_debug_keyset_replace_plan.argtypes = [sz, sz, vp, sz, vp, vp]
    lib.s2k_debug_keyset_replace_piece.argtypes = [sz]
    lib.s2k_debug_keyset_entries.argtypes = [vp, sz, ci, sz, sz, vp]
    lib.s2k_debug_keyset_section_entries.argtypes = [vp, ci, C.POINTER(sz)]
    lib.s2k_keyset_layout.argtypes = [vp]
    lib.s2k_keyset_destroy.argtypes = [vp]
    lib.s2k_keyset_destroy.restype = None
    lib.s2k_keyset_size.argtypes = [vp]
    lib.s2k_keyset_size.restype = sz
    lib.s2k_keyset_device_bytes.argtypes = [vp]
    lib.s2k_keyset_device_bytes.restype = sz
    lib.s2k_keyset_valid_keys.argtypes = [vp, vp]
    lib.s2k_ecdsa_verify_batch_keyset.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp]
    lib.s2k_ecdsa_verify_batch_keyset_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_verify_batch_keyset_submit.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_keyset_index_geometry.argtypes = [sz, u32, vp]
    lib.s2k_keyset_index_create.argtypes = [vp, u32]
    lib.s2k_keyset_index_info.argtypes = [vp, vp]
    lib.s2k_keyset_lookup.argtypes = [vp, vp, sz, vp, sz, sz, vp]
    lib.s2k_keyset_lookup_device.argtypes = [vp, vp, sz, vp, sz, sz, vp, vp]
    lib.s2k_ecdsa_verify_batch_keyset_bykey.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp]
    lib.s2k_ecdsa_verify_batch_keyset_bykey_device.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_verify_batch_keyset_bykey_submit.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_host_alloc.argtypes = [sz]
    lib.s2k_host_alloc.restype = vp
    lib.s2k_host_free.argtypes = [vp]
    lib.s2k_host_free.restype = None
    lib.s2k_host_register.argtypes = [vp, sz]
    lib.s2k_host_unregister.argtypes = [vp]
    lib.s2k_ecdsa_workspace_bytes.argtypes = [sz]
    lib.s2k_ecdsa_workspace_bytes.restype = sz
    lib.s2k_ctx_device_bytes.argtypes = [vp, sz]
    lib.s2k_ctx_device_bytes.restype = sz
    lib.s2k_parse_asn1_signature.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_char_p]
    lib.s2k_parse_compact_signature.argtypes = [C.c_char_p, sz, C.c_char_p, C.c_char_p]
    lib.s2k_is_valid_signature_encoding_bip0066.argtypes = [C.c_char_p, sz]
    lib.s2k_ecdsa_verify_encoded_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ci, sz, u32, vp]
    u64 = C.c_uint64
    lib.s2k_ecdsa_verify_batch_submit.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, C.POINTER(u64)]
    lib.s2k_ecdsa_verify_encoded_batch_submit.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ci, sz, u32, vp, C.POINTER(u64)]
    lib.s2k_ecdsa_verify_encoded_batch_keyset.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, ci, sz, u32, vp]
    lib.s2k_ecdsa_verify_encoded_batch_keyset_submit.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, ci, sz, u32, vp, C.POINTER(u64)]
    lib.s2k_ctx_last_encoded_keyset_stats.argtypes = [vp, C.POINTER(u64)]
    lib.s2k_debug_parse_encoded.argtypes = [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, sz, ci, sz, u32, ci, C.c_uint8, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.s2k_debug_parse_encoded_caps.argtypes = [vp]
    lib.s2k_digest_batch.argtypes = [vp, ci, sz, vp, vp, sz, vp, sz]
    lib.s2k_digest_batch_device.argtypes = [vp, ci, sz, vp, vp, sz, vp, sz, vp]
    lib.s2k_debug_digest_caps.argtypes = [vp]
    lib.s2k_debug_digest_strided.argtypes = [vp, ci, sz, vp, vp, sz, vp, sz, sz]
    lib.s2k_keccak_address_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.s2k_keccak_address_batch_device.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.s2k_ecdsa_recover_address_batch.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_recover_address_batch_device.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, vp, vp]
    lib.s2k_ecdsa_recover_address_messages_batch.argtypes = [vp, sz, ci, vp, vp, sz, vp, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_recover_address_messages_batch_device.argtypes = [vp, sz, ci, vp, vp, sz, vp, vp, vp, u32, vp, vp, vp]
    lib.s2k_ecdsa_verify_messages_batch.argtypes = [vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp]
    lib.s2k_ecdsa_verify_messages_batch_device.argtypes = [vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_verify_messages_batch_submit.argtypes = [vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp, C.POINTER(u64)]
    lib.s2k_ecdsa_verify_messages_batch_keyset.argtypes = [vp, vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp]
    lib.s2k_ecdsa_verify_messages_batch_keyset_device.argtypes = [vp, vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp, vp]
    lib.s2k_ecdsa_verify_messages_batch_keyset_bykey.argtypes = [vp, vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp]
    lib.s2k_ecdsa_verify_messages_batch_keyset_bykey_device.argtypes = [vp, vp, sz, vp, ci, vp, vp, sz, vp, vp, u32, vp, vp]
    lib.s2k_wait.argtypes = [vp, u64]
    lib.s2k_poll.argtypes = [vp, u64]
    lib.s2k_wait_all.argtypes = [vp]
    lib.s2k_device_count.restype = ci
    lib.s2k_group_create.argtypes = [C.POINTER(ci), sz, C.POINTER(vp)]
    lib.s2k_group_create_ex.argtypes = [C.POINTER(ci), sz, ci, u32, C.POINTER(vp)]
    lib.s2k_debug_gt_swap_in_call.argtypes = [vp, ci]
    lib.s2k_group_destroy.argtypes = [vp]
    lib.s2k_group_destroy.restype = None
    lib.s2k_group_size.argtypes = [vp]
    lib.s2k_group_size.restype = sz
    lib.s2k_group_last_error.argtypes = [vp]
    lib.s2k_group_last_error.restype = C.c_char_p
    lib.s2k_group_set_key_grouping.argtypes = [vp, ci, u32, u32, u32]
    lib.s2k_group_set_small_batch_max.argtypes = [vp, u32]
    lib.s2k_group_set_mid_batch_max.argtypes = [vp, u32]
    lib.s2k_group_set_keyset_small_batch_max.argtypes = [vp, u32]
    lib.s2k_group_set_keyset_comb_small_batch_max.argtypes = [vp, u32]
    lib.s2k_group_schnorr_batch_verify_rlc.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp]
    lib.s2k_group_multi_scalar_mult.argtypes = [vp, sz, vp, vp, vp]
    lib.s2k_group_keyset_create.argtypes = [vp, sz, vp, ci, vp]
    lib.s2k_group_keyset_create_cap.argtypes = [vp, sz, vp, ci, sz, vp]
    lib.s2k_group_keyset_capacity.argtypes = [vp]
    lib.s2k_group_keyset_capacity.restype = sz
    lib.s2k_group_keyset_reserve.argtypes = [vp, sz]
    lib.s2k_group_keyset_append.argtypes = [vp, sz, vp, C.POINTER(u32)]
    lib.s2k_group_keyset_replace.argtypes = [vp, sz, vp, vp]
    lib.s2k_group_keyset_remove.argtypes = [vp, sz, vp]
    lib.s2k_group_keyset_destroy.argtypes = [vp]
    lib.s2k_group_keyset_destroy.restype = None
    lib.s2k_group_keyset_size.argtypes = [vp]
    lib.s2k_group_keyset_size.restype = sz
    lib.s2k_group_keyset_layout.argtypes = [vp]
    lib.s2k_group_keyset_device_bytes.argtypes = [vp]
    lib.s2k_group_keyset_device_bytes.restype = sz
    lib.s2k_group_ecdsa_verify_batch_keyset.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp]
    lib.s2k_group_ecdsa_verify_batch_keyset_submit.argtypes = [vp, vp, sz, vp, vp, vp, vp, u32, vp, vp]
    lib.s2k_group_ecdsa_verify_batch.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp]
    lib.s2k_group_ecdsa_verify_batch_submit.argtypes = [vp, sz, vp, vp, vp, vp, u32, vp, C.POINTER(u64)]
    lib.s2k_group_wait.argtypes = [vp, u64]
    lib.s2k_group_ecdsa_verify_encoded_batch.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ci, sz, u32, vp]
    lib.s2k_group_ecdsa_verify_encoded_batch_submit.argtypes = [vp, sz, vp, vp, vp, vp, vp, vp, ci, sz, u32, vp, C.POINTER(u64)]
    lib.s2k_group_member_stats.argtypes = [vp, vp]
    lib.s2k_schnorr_verify_batch.argtypes = [vp, sz, vp, vp, vp, sz, vp, u32, vp]
    lib.s2k_schnorr_verify_batch_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, u32, vp, vp]
    lib.s2k_schnorr_verify_batch_keyset.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, u32, vp]
    lib.s2k_schnorr_verify_batch_keyset_device.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, u32, vp, vp]
    lib.s2k_schnorr_verify_batch_keyset_submit.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, u32, vp, vp]
    lib.s2k_schnorr_verify_batch_keyset_bykey.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, u32, vp]
    lib.s2k_schnorr_verify_batch_keyset_bykey_device.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, u32, vp, vp]
    lib.s2k_schnorr_verify_batch_keyset_bykey_submit.argtypes = [vp, vp, sz, vp, vp, vp, sz, vp, u32, vp, vp]
    lib.s2k_schnorr_batch_verify_rlc.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, C.POINTER(ci)]
    lib.s2k_schnorr_batch_verify_rlc_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, C.POINTER(ci), vp]
    lib.s2k_schnorr_verify_batch_bisect.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.s2k_schnorr_verify_batch_bisect_device.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp]
    lib.s2k_scalar_base_mult_batch.argtypes = [vp, sz, vp, vp]
    lib.s2k_scalar_mult_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.s2k_double_scalar_mult_basepoint_batch.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.s2k_double_scalar_mult_basepoint_batch_ex.argtypes = [vp, u32, sz, vp, vp, vp, vp]
    lib.s2k_fp_op_batch_ex.argtypes = [vp, u32, ci, u32, sz, vp, vp, vp, vp]
    lib.s2k_fp_op_batch_ex8.argtypes = [vp, u32, ci, u32, u32, sz, vp, vp, vp, vp]
    lib.s2k_fn_split_glv_batch_ex.argtypes = [vp, u32, sz, vp, vp, vp, vp]
    lib.s2k_point_add_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.s2k_point_double_batch.argtypes = [vp, sz, vp, vp]
    lib.s2k_point_decode_batch.argtypes = [vp, sz, sz, vp, vp, vp]
    lib.s2k_multi_scalar_mult.argtypes = [vp, sz, vp, vp, vp]
    lib.s2k_multi_scalar_mult_device.argtypes = [vp, sz, vp, vp, vp, vp]
    lib.s2k_debug_msm_terms.argtypes = [vp, sz, vp, vp, vp, ci, vp, vp, vp, sz, vp, sz]
    lib.s2k_debug_schnorr_rlc_point.argtypes = [vp, sz, vp, vp, vp, sz, vp, vp, ci, sz, sz, vp, vp, vp]
    lib.s2k_debug_ecdsa_rlc_point.argtypes = [vp, sz, vp, vp, vp, vp, vp, u32, vp, ci, sz, sz, vp, vp, vp]
    lib.s2k_multi_scalar_mult_segments.argtypes = [vp, sz, vp, vp, sz, vp, vp]
    lib.s2k_multi_scalar_mult_segments_device.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp]
    lib.s2k_debug_msm_segments_plan.argtypes = [sz, sz, vp, u32, C.c_uint64, vp, sz, vp, vp, vp, vp]
    lib.s2k_pointset_create.argtypes = [vp, sz, vp, ci, C.POINTER(vp)]
    lib.s2k_pointset_destroy.argtypes = [vp]
    lib.s2k_pointset_destroy.restype = None
    lib.s2k_pointset_size.argtypes = [vp]
    lib.s2k_pointset_size.restype = sz
    lib.s2k_pointset_window_bits.argtypes = [vp]
    lib.s2k_pointset_device_bytes.argtypes = [vp]
    lib.s2k_pointset_device_bytes.restype = sz
    lib.s2k_pointset_geometry.argtypes = [ci, vp]
    lib.s2k_keyset_geometry.argtypes = [ci, vp]
    lib.s2k_debug_pointset_entry.argtypes = [vp, sz, C.c_uint, C.c_uint, vp]
    lib.s2k_debug_pointset_check_args.argtypes = [sz, sz, ci, sz, vp]
    lib.s2k_pointset_multi_scalar_mult_segments.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp]
    lib.s2k_pointset_multi_scalar_mult_segments_device.argtypes = [vp, vp, sz, vp, vp, sz, vp, vp, vp]
    lib.s2k_h2c_dst_prime.argtypes = [C.c_char_p, sz, C.c_char_p, C.POINTER(sz)]
    lib.s2k_expand_message_xmd_batch.argtypes = [vp, sz, C.c_char_p, sz, vp, vp, sz, sz, vp]
    lib.s2k_map_to_curve_batch.argtypes = [vp, sz, sz, sz, vp, vp]
    lib.s2k_hash_to_curve_batch.argtypes = [vp, ci, sz, C.c_char_p, sz, vp, vp, sz, vp]
    lib.s2k_hash_to_curve_batch_device.argtypes = [vp, ci, sz, C.c_char_p, sz, vp, vp, sz, sz, vp, vp]
    lib.s2k_fp_op_batch.argtypes = [vp, ci, sz, vp, vp, vp, vp]
    lib.s2k_fn_op_batch.argtypes = [vp, ci, sz, vp, vp, vp, vp]
    lib.s2k_fn_split_glv_batch.argtypes = [vp, sz, vp, vp, vp]
    lib.s2k_debug_gtable_entry.argtypes = [vp, C.c_uint, C.c_uint, vp]
    lib.s2k_ct_scalar_mult.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    lib.s2k_ct_scalar_base_mult.argtypes = [C.c_char_p, C.c_char_p]
    lib.s2k_ct_ecdh.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    lib.s2k_ct_debug_fe_mul_count.restype = C.c_uint64
    cp, pu64 = C.c_char_p, C.POINTER(C.c_uint64)
    lib.s2k_ct_point_add.argtypes = [cp, cp, cp]
    lib.s2k_ct_point_double.argtypes = [cp, cp]
    lib.s2k_ct_point_subtract.argtypes = [cp, cp, cp]
    lib.s2k_ct_point_negate.argtypes = [cp, cp]
    lib.s2k_ct_point_conditional_negate.argtypes = [cp, C.c_uint64, cp]
    lib.s2k_ct_point_conditional_select.argtypes = [cp, cp, C.c_uint64, cp]
    lib.s2k_ct_point_equal.argtypes = [cp, cp, pu64]
    lib.s2k_ct_point_is_identity.argtypes = [cp, pu64]
    lib.s2k_ct_point_is_y_odd.argtypes = [cp, pu64]
    lib.s2k_ct_scalar_op.argtypes = [ci, cp, cp, cp]
    lib.s2k_ct_scalar_conditional_select.argtypes = [cp, cp, C.c_uint64, cp]
    lib.s2k_ct_scalar_conditional_negate.argtypes = [cp, C.c_uint64, cp]
    lib.s2k_ct_scalar_predicate.argtypes = [ci, cp, cp, pu64]
    lib.s2k_ct_scalar_set_bytes.argtypes = [cp, cp, pu64]
    lib.s2k_ct_fe_op.argtypes = [ci, cp, cp, cp, pu64]
    lib.s2k_ct_multi_scalar_mult.argtypes = [sz, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.s2k_device_pci_bus_id.argtypes = [ci, C.c_char_p, sz]
    lib.s2k_device_numa_node.argtypes = [ci]
    lib.s2k_bind_thread_to_node.argtypes = [ci]
    lib.s2k_topology_prefer_node.argtypes = [vp, sz, ci]
    lib.s2k_topology_node_count.argtypes = [C.c_char_p]
    lib.s2k_topology_numa_node_of_pci.argtypes = [C.c_char_p, C.c_char_p]
    lib.s2k_topology_node_cpus.argtypes = [C.c_char_p, ci, C.POINTER(ci), sz]
    lib.s2k_ctx_ticket_timing.argtypes = [vp, ci]
    lib.s2k_ticket_times.argtypes = [vp, C.c_uint64, C.POINTER(C.c_double)]
    lib.s2k_group_member_stats_ex.argtypes = [vp, vp]
    lib.s2k_group_gt_wait.argtypes = [vp]
    lib.s2k_group_shard_size.argtypes = [vp, sz]
    lib.s2k_group_shard_size.restype = sz
    lib.s2k_group_host_alloc.argtypes = [vp, sz, sz]
    lib.s2k_group_host_alloc.restype = vp
    lib.s2k_group_host_free.argtypes = [vp, vp]
    lib.s2k_group_host_free.restype = None
    lib.s2k_ctx_set_small_batch_max.argtypes = [vp, u32]
    lib.s2k_ctx_set_mid_batch_max.argtypes = [vp, u32]
    lib.s2k_ctx_set_keyset_small_batch_max.argtypes = [vp, u32]
    lib.s2k_ctx_set_keyset_comb_small_batch_max.argtypes = [vp, u32]
    lib.s2k_ctx_last_keyset_ladder.argtypes = [vp]
    lib.s2k_ctx_create_ex.argtypes = [ci, ci, u32, C.POINTER(vp)]
    lib.s2k_set_generator_table_budget.argtypes = [sz]
    lib.s2k_set_generator_table_budget.restype = None
    lib.s2k_set_table_memory_budgets.argtypes = [sz, sz]
    lib.s2k_set_table_memory_budgets.restype = None
    lib.s2k_ctx_gt_info.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.s2k_ctx_gt_note.argtypes = [vp]
    lib.s2k_ctx_gt_note.restype = C.c_char_p
    lib.s2k_ctx_gt_wait.argtypes = [vp]
    lib.s2k_ct_ecdsa_sign_raw.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint8)]
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "s2k_ctx_create", "s2k_ctx_destroy", "s2k_last_error", "s2k_version", "s2k_build_config",
    "s2k_ctx_profile", "s2k_ctx_profile_read", "s2k_ctx_profile_read_stages", "s2k_ctx_profile_msm", "s2k_ctx_profile_read_msm",
    "s2k_ctx_set_key_grouping", "s2k_ctx_set_keyed_ladder", "s2k_ctx_last_keyed_ladder", "s2k_ctx_key_grouping_stats", "s2k_ctx_key_grouping_adaptive",
    "s2k_ecdsa_verify_batch", "s2k_ecdsa_verify_batch_device", "s2k_ecdsa_workspace_bytes", "s2k_ctx_device_bytes",
    "s2k_keyset_create", "s2k_keyset_create_ex", "s2k_keyset_layout", "s2k_keyset_geometry", "s2k_keyset_destroy", "s2k_keyset_size", "s2k_keyset_device_bytes", "s2k_keyset_valid_keys",
    "s2k_keyset_create_cap", "s2k_keyset_capacity", "s2k_keyset_reserve", "s2k_keyset_append", "s2k_keyset_append_device",
    "s2k_keyset_replace", "s2k_keyset_replace_device", "s2k_keyset_remove", "s2k_debug_keyset_replace_plan", "s2k_debug_keyset_replace_piece",
    "s2k_debug_keyset_entries", "s2k_debug_keyset_section_entries",
    "s2k_ecdsa_verify_batch_keyset", "s2k_ecdsa_verify_batch_keyset_device", "s2k_ecdsa_verify_batch_keyset_submit",
    "s2k_keyset_index_geometry", "s2k_keyset_index_create", "s2k_keyset_index_info", "s2k_keyset_lookup", "s2k_keyset_lookup_device",
    "s2k_ecdsa_verify_batch_keyset_bykey", "s2k_ecdsa_verify_batch_keyset_bykey_device", "s2k_ecdsa_verify_batch_keyset_bykey_submit",
    "s2k_schnorr_verify_batch_keyset_bykey", "s2k_schnorr_verify_batch_keyset_bykey_device", "s2k_schnorr_verify_batch_keyset_bykey_submit",
    "s2k_pack_valid_device", "s2k_host_alloc", "s2k_host_free", "s2k_host_register", "s2k_host_unregister", "s2k_ecdsa_recover_batch", "s2k_ecdsa_recover_batch_device",
    "s2k_ecdsa_batch_verify_rlc", "s2k_ecdsa_batch_verify_rlc_device",
    "s2k_ecdsa_verify_recoverable_batch_bisect", "s2k_ecdsa_verify_recoverable_batch_bisect_device",
    "s2k_parse_asn1_signature", "s2k_parse_compact_signature", "s2k_is_valid_signature_encoding_bip0066",
    "s2k_ecdsa_verify_encoded_batch",
    "s2k_ecdsa_verify_encoded_batch_keyset", "s2k_ecdsa_verify_encoded_batch_keyset_submit", "s2k_ctx_last_encoded_keyset_stats",
    "s2k_debug_parse_encoded", "s2k_debug_parse_encoded_caps",
    "s2k_digest_batch", "s2k_digest_batch_device", "s2k_debug_digest_caps", "s2k_debug_digest_strided",
    "s2k_ecdsa_verify_messages_batch", "s2k_ecdsa_verify_messages_batch_device", "s2k_ecdsa_verify_messages_batch_submit",
    "s2k_ecdsa_verify_messages_batch_keyset", "s2k_ecdsa_verify_messages_batch_keyset_device",
    "s2k_ecdsa_verify_messages_batch_keyset_bykey", "s2k_ecdsa_verify_messages_batch_keyset_bykey_device",
    "s2k_keccak_address_batch", "s2k_keccak_address_batch_device", "s2k_ecdsa_recover_address_batch", "s2k_ecdsa_recover_address_batch_device",
    "s2k_ecdsa_recover_address_messages_batch", "s2k_ecdsa_recover_address_messages_batch_device",
    "s2k_ecdsa_verify_batch_submit", "s2k_ecdsa_verify_encoded_batch_submit", "s2k_wait", "s2k_poll", "s2k_wait_all",
    "s2k_device_count", "s2k_group_create", "s2k_group_destroy", "s2k_group_size", "s2k_group_last_error",
    "s2k_group_set_key_grouping", "s2k_group_set_small_batch_max", "s2k_group_set_mid_batch_max", "s2k_group_ecdsa_verify_batch", "s2k_group_ecdsa_verify_batch_submit", "s2k_group_wait",
    "s2k_group_ecdsa_verify_encoded_batch", "s2k_group_ecdsa_verify_encoded_batch_submit",
    "s2k_group_member_stats", "s2k_group_schnorr_batch_verify_rlc", "s2k_group_multi_scalar_mult",
    "s2k_group_keyset_create", "s2k_group_keyset_destroy", "s2k_group_keyset_size", "s2k_group_keyset_layout", "s2k_group_keyset_device_bytes",
    "s2k_group_keyset_create_cap", "s2k_group_keyset_capacity", "s2k_group_keyset_reserve", "s2k_group_keyset_append",
    "s2k_group_keyset_replace", "s2k_group_keyset_remove",
    "s2k_group_ecdsa_verify_batch_keyset", "s2k_group_ecdsa_verify_batch_keyset_submit",
    "s2k_schnorr_verify_batch", "s2k_schnorr_verify_batch_device",
    "s2k_schnorr_verify_batch_keyset", "s2k_schnorr_verify_batch_keyset_device", "s2k_schnorr_verify_batch_keyset_submit",
    "s2k_schnorr_batch_verify_rlc", "s2k_schnorr_batch_verify_rlc_device",
    "s2k_schnorr_verify_batch_bisect", "s2k_schnorr_verify_batch_bisect_device",
    "s2k_scalar_base_mult_batch", "s2k_scalar_mult_batch", "s2k_double_scalar_mult_basepoint_batch",
    "s2k_point_add_batch", "s2k_point_double_batch", "s2k_point_decode_batch",
    "s2k_multi_scalar_mult", "s2k_multi_scalar_mult_device", "s2k_debug_msm_terms",
    "s2k_debug_schnorr_rlc_point", "s2k_debug_ecdsa_rlc_point",
    "s2k_multi_scalar_mult_segments", "s2k_multi_scalar_mult_segments_device", "s2k_debug_msm_segments_plan",
    "s2k_pointset_create", "s2k_pointset_destroy", "s2k_pointset_size", "s2k_pointset_window_bits", "s2k_pointset_device_bytes",
    "s2k_pointset_geometry", "s2k_debug_pointset_entry", "s2k_debug_pointset_check_args",
    "s2k_pointset_multi_scalar_mult_segments", "s2k_pointset_multi_scalar_mult_segments_device",
    "s2k_h2c_dst_prime", "s2k_expand_message_xmd_batch", "s2k_map_to_curve_batch", "s2k_hash_to_curve_batch", "s2k_hash_to_curve_batch_device",
    "s2k_fp_op_batch", "s2k_fn_op_batch", "s2k_fn_split_glv_batch", "s2k_debug_gtable_entry", "s2k_generator_window_bits",
    "s2k_double_scalar_mult_basepoint_batch_ex", "s2k_fp_op_batch_ex", "s2k_fp_op_batch_ex8", "s2k_fn_split_glv_batch_ex",
    "s2k_ct_scalar_mult", "s2k_ct_scalar_base_mult", "s2k_ct_ecdh", "s2k_ct_ecdsa_sign_raw", "s2k_ct_debug_fe_mul_count",
    "s2k_ct_multi_scalar_mult",
    "s2k_device_pci_bus_id", "s2k_device_numa_node", "s2k_bind_thread_to_node", "s2k_topology_prefer_node", "s2k_topology_node_count",
    "s2k_topology_numa_node_of_pci", "s2k_topology_node_cpus", "s2k_ctx_ticket_timing", "s2k_ticket_times",
    "s2k_group_member_stats_ex", "s2k_group_gt_wait", "s2k_group_shard_size", "s2k_group_host_alloc", "s2k_group_host_free",
    "s2k_ctx_set_small_batch_max", "s2k_ctx_set_mid_batch_max", "s2k_ctx_create_ex", "s2k_set_generator_table_budget", "s2k_set_table_memory_budgets", "s2k_ctx_gt_info", "s2k_ctx_gt_note", "s2k_ctx_gt_wait",
    "s2k_group_create_ex", "s2k_debug_gt_swap_in_call",
    "s2k_ctx_set_keyset_small_batch_max", "s2k_ctx_last_keyset_ladder", "s2k_group_set_keyset_small_batch_max",
    "s2k_ctx_set_keyset_comb_small_batch_max", "s2k_group_set_keyset_comb_small_batch_max",
    "s2k_ct_point_add", "s2k_ct_point_double", "s2k_ct_point_subtract", "s2k_ct_point_negate", "s2k_ct_point_conditional_negate",
    "s2k_ct_point_conditional_select", "s2k_ct_point_equal", "s2k_ct_point_is_identity", "s2k_ct_point_is_y_odd",
    "s2k_ct_scalar_op", "s2k_ct_scalar_conditional_select", "s2k_ct_scalar_conditional_negate", "s2k_ct_scalar_predicate",
    "s2k_ct_scalar_set_bytes", "s2k_ct_fe_op",
]


def _arr(x, width, n=None):
    """bytes / list of bytes / ndarray -> contiguous uint8 array of shape (n, width)."""
    if isinstance(x, (list, tuple)):
        x = b"".join(x)
    if isinstance(x, (bytes, bytearray, memoryview)):
        a = np.frombuffer(bytes(x), dtype=np.uint8)
    else:
        a = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
    if a.size % width:
        raise ValueError(f"buffer length {a.size} is not a multiple of {width}")
    a = a.reshape(-1, width)
    if n is not None and a.shape[0] != n:
        # the reference panics on length mismatch (point_mul_multi.go:27-29)
        raise ValueError(f"length mismatch: expected {n} items, got {a.shape[0]}")
    return np.ascontiguousarray(a)


# ---- host-side parsing (no GPU needed) --------------------------------------------------------
def parse_asn1_signature(der: bytes):
    """ParseASN1Signature (secec/s11n.go:83): (r, s) as 32-byte strings, or None."""
    r, s = C.create_string_buffer(32), C.create_string_buffer(32)
    return (r.raw, s.raw) if load_library().s2k_parse_asn1_signature(der, len(der), r, s) == 0 else None


def parse_compact_signature(sig: bytes):
    """ParseCompactSignature (secec/s11n.go:129)."""
    r, s = C.create_string_buffer(32), C.create_string_buffer(32)
    return (r.raw, s.raw) if load_library().s2k_parse_compact_signature(sig, len(sig), r, s) == 0 else None


def is_valid_signature_encoding_bip0066(sig: bytes) -> bool:
    """bitcoin.IsValidSignatureEncodingBIP0066 (secec/bitcoin/asn1_shitcoin.go:13)."""
    return bool(load_library().s2k_is_valid_signature_encoding_bip0066(sig, len(sig)))


# ---- constant-time twins on the host CPU (no GPU needed) -------------------------------------
def ct_scalar_mult(k: bytes, point65: bytes):
    """Point.ScalarMult (point_mul_glv.go:257), constant time, CPU.  Returns the 65-byte record or None
    for a malformed point."""
    out = C.create_string_buffer(65)
    return out.raw if load_library().s2k_ct_scalar_mult(bytes(k), bytes(point65), out) == 0 else None


def h2c_dst_prime(dst: bytes) -> bytes:
    """DST_prime of expand_message_xmd (s2k_h2c_dst_prime; h2c_expand_message.go:46-63): dst || len(dst), a tag of more than
    255 bytes hashed first.  Host only.  An empty tag raises ValueError (the reference returns errInvalidDomainSep)."""
    dst = bytes(dst)
    if len(dst) == 0:
        raise ValueError("secp256k1/secec/h2c: invalid domain separator")
    out, n = C.create_string_buffer(256), C.c_size_t(0)
    rc = load_library().s2k_h2c_dst_prime(dst, len(dst), out, C.byref(n))
    if rc != 0:
        raise EngineError(f"s2k_h2c_dst_prime failed ({rc})")
    return out.raw[:n.value]


def _h2c_messages(msgs):
    """A list of byte strings or a (blob, offsets) pair -> (n, contiguous uint8 blob, uint64 offsets); ValueError for offsets
    that do not start at 0, decrease or leave the blob (what the C-ABI would refuse, or could not check)."""
    if isinstance(msgs, tuple) and len(msgs) == 2 and not isinstance(msgs[0], (bytes, bytearray)):
        blob = np.ascontiguousarray(msgs[0], dtype=np.uint8).reshape(-1)
        raw = np.asarray(msgs[1])
        if raw.ndim != 1 or raw.shape[0] < 1 or raw.dtype.kind not in "iu" or (raw.dtype.kind == "i" and int(raw.min()) < 0):
            raise ValueError("offsets must be a one-dimensional array of n + 1 non-negative integers")
        offs = np.ascontiguousarray(raw, dtype=np.uint64)
        if int(offs[0]) != 0 or bool(np.any(offs[1:] < offs[:-1])):
            raise ValueError("offsets must start at 0 and must not decrease")
        if int(offs[-1]) > blob.size:
            raise ValueError(f"offsets end at {int(offs[-1])}, the message buffer holds {blob.size} bytes")
        if blob.size == 0:
            blob = np.zeros(1, dtype=np.uint8)
        return offs.shape[0] - 1, blob, offs
    blob, offs = _concat([bytes(m) for m in msgs])
    return len(offs) - 1, blob, offs


def _h2c_dst(dst) -> bytes:
    dst = bytes(dst)
    if len(dst) == 0:
        raise ValueError("secp256k1/secec/h2c: invalid domain separator")
    return dst


def check_segment_offsets(offsets, n: int) -> np.ndarray:
    """Segment offsets as the contiguous uint64 array the C-ABI takes; ValueError unless they start at 0, never decrease
    and end at n (what s2k_multi_scalar_mult_segments would refuse with S2K_ERR_ARG)."""
    raw = np.asarray(offsets)
    if raw.ndim != 1 or raw.shape[0] < 1:
        raise ValueError("offsets must be a one-dimensional array of n_seg + 1 entries")
    if raw.dtype.kind not in "iu" or (raw.dtype.kind == "i" and raw.size and int(raw.min()) < 0):
        raise ValueError("offsets must be non-negative integers")
    off = np.ascontiguousarray(raw, dtype=np.uint64)
    if int(off[0]) != 0:
        raise ValueError("offsets must start at 0")
    if off.shape[0] > 1 and bool(np.any(off[1:] < off[:-1])):
        raise ValueError("offsets must not decrease")
    if int(off[-1]) != int(n):
        raise ValueError(f"offsets must end at the number of terms ({int(off[-1])} != {int(n)})")
    return off


def pointset_geometry(window_bits: int) -> tuple:
    """(digit positions, entries per position, table bytes per point) of a point set at 4- or 8-bit digits
    (s2k_pointset_geometry; no device).  ValueError for any other width."""
    out = np.zeros(3, dtype=np.uint64)
    if load_library().s2k_pointset_geometry(int(window_bits), out.ctypes.data) != 0:
        raise ValueError("secp256k1: point-set digit width is 4 or 8")
    return tuple(int(x) for x in out)


def parse_encoded_caps() -> tuple:
    """(key, digest, signature) bytes of LDS the parse kernels of the encoded calls stage a workgroup's stretch of each blob in
    (s2k_debug_parse_encoded_caps; no device)."""
    out = np.zeros(3, dtype=np.uint32)
    if load_library().s2k_debug_parse_encoded_caps(out.ctypes.data) != 0:
        raise EngineError("s2k_debug_parse_encoded_caps failed")
    return tuple(int(v) for v in out)


def digest_caps() -> int:
    """Bytes of LDS the digest kernel stages a workgroup's stretch of messages in (s2k_debug_digest_caps; no device)."""
    out = np.zeros(1, dtype=np.uint32)
    if load_library().s2k_debug_digest_caps(out.ctypes.data) != 0:
        raise EngineError("s2k_debug_digest_caps failed")
    return int(out[0])


def _messages(msgs, n=None):
    """Messages as the calls that hash on the device take them: a list of byte strings, a (blob, offsets) pair - blob a bytes
    object or uint8 array, offsets n + 1 byte offsets into it, used as they are - or an (n, L) uint8 array of fixed-length
    messages.  Returns (n, blob address or None, offsets address or None, msg_len, arrays to keep alive)."""
    if isinstance(msgs, tuple) and len(msgs) == 2 and isinstance(msgs[1], (np.ndarray, list)):
        blob, offs = msgs
        if isinstance(blob, (bytes, bytearray, memoryview)):
            blob = np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8)
        elif not (isinstance(blob, np.ndarray) and blob.dtype == np.uint8 and blob.flags["C_CONTIGUOUS"]):
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
        if not (isinstance(offs, np.ndarray) and offs.dtype == np.uint64 and offs.flags["C_CONTIGUOUS"]):
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if offs.shape[0] < 1:
            raise ValueError("offsets: n + 1 entries are needed")
        m, keep = offs.shape[0] - 1, [blob, offs]
        ret = (blob.ctypes.data if blob.size else None, offs.ctypes.data, 0)
    elif isinstance(msgs, (list, tuple)):
        offs = np.zeros(len(msgs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in msgs], dtype=np.uint64)
        blob = np.frombuffer(b"".join(bytes(x) for x in msgs) or b"\0", dtype=np.uint8)
        m, keep = len(msgs), [blob, offs]
        ret = (blob.ctypes.data, offs.ctypes.data, 0)
    else:
        a = msgs if (isinstance(msgs, np.ndarray) and msgs.dtype == np.uint8 and msgs.flags["C_CONTIGUOUS"]) else np.ascontiguousarray(msgs, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("fixed-length messages: an (n, L) uint8 array is needed")
        m, keep = a.shape[0], [a]
        ret = (a.ctypes.data if a.size else None, None, a.shape[1])
    if n is not None and m != n:
        raise ValueError(f"length mismatch: expected {n} messages, got {m}")
    return (m,) + ret + (keep,)


def keyset_geometry(layout: int) -> tuple:
    """(table additions per signature, doublings per signature, table bytes per key) of a key-set layout, KEYSET_CHUNKS ..
    KEYSET_COMB (s2k_keyset_geometry; no device).  ValueError for KEYSET_AUTO and unknown layouts."""
    out = np.zeros(3, dtype=np.uint64)
    if load_library().s2k_keyset_geometry(int(layout), out.ctypes.data) != 0:
        raise ValueError("secp256k1: key-set layout without a fixed geometry")
    return tuple(int(x) for x in out)


def keyset_index_geometry(n_keys: int, log2_slots: int = 0) -> tuple:
    """(slots, bytes) of the index of a key set of n_keys keys (s2k_keyset_index_geometry; no device); log2_slots 0: the
    power of two >= 2 * n_keys, at least 16.  ValueError when 2^log2_slots <= n_keys, log2_slots > 31 or n_keys is 0."""
    out = np.zeros(2, dtype=np.uint64)
    if int(n_keys) < 0 or not 0 <= int(log2_slots) < 1 << 32 or \
            load_library().s2k_keyset_index_geometry(int(n_keys), int(log2_slots), out.ctypes.data) != 0:
        raise ValueError(f"no key-set index of {n_keys} keys in 2^{log2_slots} slots")
    return int(out[0]), int(out[1])


def _slots(slots) -> np.ndarray:
    """row numbers of a key set -> contiguous uint32 array (ValueError for what is no list of uint32 values)"""
    a = np.asarray(slots)
    if a.size and (a.dtype.kind not in "iu" or int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise ValueError("secp256k1: slots are uint32 row numbers")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)


def keyset_replace_plan(n_live: int, slots, piece_keys: int = 0) -> dict:
    """The host-side plan of KeySet.replace / remove (s2k_debug_keyset_replace_plan; no device): the argument checks
    (EngineError for a slot >= n_live or one named twice), `order` - the positions in `slots` in ascending order of the slot -
    and the number of pieces of at most piece_keys slots (0: one piece)."""
    lib = load_library()
    slots = _slots(slots)
    m = slots.shape[0]
    order = np.zeros(m, dtype=np.uint32)
    pieces = C.c_uint64(0)
    rc = lib.s2k_debug_keyset_replace_plan(int(n_live), m, slots.ctypes.data if m else None, int(piece_keys), order.ctypes.data if m else None,
                                           C.addressof(pieces))
    if rc:
        raise EngineError(f"s2k error {rc}: {lib.s2k_last_error(None).decode()}")
    return dict(order=order, pieces=int(pieces.value))


def debug_keyset_replace_piece(keys: int) -> None:
    """Test knob (s2k_debug_keyset_replace_piece): KeySet.replace / remove work in pieces of `keys` keys; 0: automatic."""
    load_library().s2k_debug_keyset_replace_piece(int(keys))


def msm_segments_plan(n: int, offsets, piece_terms: int = 0, crossover: int = 0, arrays: bool = True) -> dict:
    """The host-side plan of multi_scalar_mult_segments (s2k_debug_msm_segments_plan; no device).  `offsets` goes to the library
    as it is (a uint64 array): its argument checks are part of what this exposes.  EngineError on refused arguments."""
    lib = load_library()
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n_seg = max(off.shape[0] - 1, 0)
    summary = np.zeros(8, dtype=np.uint64)
    optr = off.ctypes.data if off.shape[0] else None
    rc = lib.s2k_debug_msm_segments_plan(int(n), n_seg, optr, int(piece_terms), int(crossover), summary.ctypes.data, 0, None, None, None, None)
    if rc:
        raise EngineError(f"s2k_debug_msm_segments_plan: {rc}")
    keys = ("pieces", "long_segments", "short_terms", "workspace_bytes", "max_long", "piece_terms", "crossover", "runs")
    plan = {k: int(v) for k, v in zip(keys, summary)}
    if arrays:
        npc = plan["pieces"]
        first, ln, dest = (np.zeros(max(npc, 1), dtype=np.uint32) for _ in range(3))
        desc = np.zeros(max(2 * n_seg, 1), dtype=np.uint32)
        rc = lib.s2k_debug_msm_segments_plan(int(n), n_seg, optr, int(piece_terms), int(crossover), summary.ctypes.data, npc,
                                             first.ctypes.data, ln.ctypes.data, dest.ctypes.data, desc.ctypes.data)
        if rc:
            raise EngineError(f"s2k_debug_msm_segments_plan: {rc}")
        plan.update(piece_first=first[:npc], piece_len=ln[:npc], piece_dest=dest[:npc], seg_desc=desc[:2 * n_seg].reshape(n_seg, 2))
    return plan


def ct_multi_scalar_mult(scalars, points):
    """Point.MultiScalarMult (point_mul_multi.go:25-67), constant time in the scalars, CPU: Straus with masked table
    scans; one term is Point.ScalarMult, none is the identity.  `scalars`: 32-byte strings, `points`: 65-byte records.
    Returns the 65-byte record of the sum, or None for a malformed point.  A length mismatch raises (the reference
    panics, :27-29)."""
    scalars, points = [bytes(x) for x in scalars], [bytes(x) for x in points]
    if len(scalars) != len(points):
        raise ValueError("secp256k1: len(scalars) != len(points)")
    if any(len(x) != 32 for x in scalars) or any(len(x) != 65 for x in points):
        raise ValueError("scalars are 32 bytes, point records 65")
    out = C.create_string_buffer(65)
    rc = load_library().s2k_ct_multi_scalar_mult(len(scalars), b"".join(scalars) or None, b"".join(points) or None, out)
    if rc == -4:
        raise MemoryError("s2k_ct_multi_scalar_mult: out of memory")
    return out.raw if rc == 0 else None


# ---- single operations, constant time, host CPU (s2k_ct_point_* / s2k_ct_scalar_* / s2k_ct_fe_op): what the reference's
# Point / Scalar / field.Element methods bind to.  A malformed operand raises ValueError (the reference's constructors fail).
def _ct_out(fn, n, *args):
    out = C.create_string_buffer(n)
    rc = fn(*args, out)
    if rc != 0:
        raise ValueError(f"{fn.__name__}: operand the reference's type cannot hold ({rc})")
    return out.raw


def _ct_flag(fn, *args) -> int:
    v = C.c_uint64(7)
    rc = fn(*args, C.byref(v))
    if rc != 0:
        raise ValueError(f"{fn.__name__}: operand the reference's type cannot hold ({rc})")
    return int(v.value)


def ct_point_add(a65, b65): return _ct_out(load_library().s2k_ct_point_add, 65, bytes(a65), bytes(b65))
def ct_point_double(a65): return _ct_out(load_library().s2k_ct_point_double, 65, bytes(a65))
def ct_point_subtract(a65, b65): return _ct_out(load_library().s2k_ct_point_subtract, 65, bytes(a65), bytes(b65))
def ct_point_negate(a65): return _ct_out(load_library().s2k_ct_point_negate, 65, bytes(a65))
def ct_point_conditional_negate(a65, ctrl): return _ct_out(load_library().s2k_ct_point_conditional_negate, 65, bytes(a65), int(ctrl))
def ct_point_conditional_select(a65, b65, ctrl): return _ct_out(load_library().s2k_ct_point_conditional_select, 65, bytes(a65), bytes(b65), int(ctrl))
def ct_point_equal(a65, b65): return _ct_flag(load_library().s2k_ct_point_equal, bytes(a65), bytes(b65))
def ct_point_is_identity(a65): return _ct_flag(load_library().s2k_ct_point_is_identity, bytes(a65))
def ct_point_is_y_odd(a65): return _ct_flag(load_library().s2k_ct_point_is_y_odd, bytes(a65))
def ct_scalar_op(op, a32, b32=None): return _ct_out(load_library().s2k_ct_scalar_op, 32, int(op), bytes(a32), None if b32 is None else bytes(b32))
def ct_scalar_conditional_select(a32, b32, ctrl): return _ct_out(load_library().s2k_ct_scalar_conditional_select, 32, bytes(a32), bytes(b32), int(ctrl))
def ct_scalar_conditional_negate(a32, ctrl): return _ct_out(load_library().s2k_ct_scalar_conditional_negate, 32, bytes(a32), int(ctrl))
def ct_scalar_predicate(what, a32, b32=None): return _ct_flag(load_library().s2k_ct_scalar_predicate, int(what), bytes(a32), None if b32 is None else bytes(b32))


def ct_scalar_set_bytes(src32):
    """Scalar.SetBytes -> (src mod n, did_reduce)"""
    out, did = C.create_string_buffer(32), C.c_uint64(7)
    if load_library().s2k_ct_scalar_set_bytes(bytes(src32), out, C.byref(did)) != 0:
        raise ValueError("s2k_ct_scalar_set_bytes")
    return out.raw, int(did.value)


def ct_fe_op(op, a32, b32=None):
    """field.Element operation -> (out, flag); flag is 1 except for OP_SQRT of a non-square"""
    out, flag = C.create_string_buffer(32), C.c_uint64(7)
    rc = load_library().s2k_ct_fe_op(int(op), bytes(a32), None if b32 is None else bytes(b32), out, C.byref(flag))
    if rc != 0:
        raise ValueError(f"s2k_ct_fe_op: operand the reference's type cannot hold ({rc})")
    return out.raw, int(flag.value)


def ct_scalar_base_mult(k: bytes) -> bytes:
    """Point.ScalarBaseMult (point_mul_table.go:168), constant time, CPU."""
    out = C.create_string_buffer(65)
    rc = load_library().s2k_ct_scalar_base_mult(bytes(k), out)
    if rc != 0:
        raise EngineError(f"s2k_ct_scalar_base_mult failed ({rc})")
    return out.raw


def ct_ecdh(priv32: bytes, pub65: bytes):
    """PrivateKey.ECDH (secec/secec.go:53): the shared x-coordinate, or None for invalid inputs."""
    out = C.create_string_buffer(32)
    return out.raw if load_library().s2k_ct_ecdh(bytes(priv32), bytes(pub65), out) == 0 else None


def ct_ecdsa_sign_raw(priv32: bytes, digest32: bytes, nonce32: bytes):
    """(r, s, recovery_id) for a caller-supplied nonce (secec/ecdsa.go:335-390), or None when the
    nonce has to be redrawn."""
    r, s, rid = C.create_string_buffer(32), C.create_string_buffer(32), C.c_uint8(0)
    rc = load_library().s2k_ct_ecdsa_sign_raw(bytes(priv32), bytes(digest32), bytes(nonce32), r, s, C.byref(rid))
    return (r.raw, s.raw, int(rid.value)) if rc == 0 else None


def _concat(items):
    offs = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        offs[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    blob = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
    return blob, offs


def _out_array(out, n):
    """The verdict array of a submit call: a fresh one, or the caller's - which the library writes n bytes into, later, from
    another thread: it has to be exactly a writable C-contiguous uint8 array of n items."""
    if out is None:
        return np.zeros(n, dtype=np.uint8)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.shape == (n,) and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]):
        raise ValueError(f"out must be a writable C-contiguous uint8 array of shape ({n},)")
    return out


class _TicketOwner:
    """Keeps the buffers of the batches in flight alive.  The library reads the inputs and writes the verdicts of a ticket
    asynchronously (DMA from pinned arrays; s2k_internal_pipe_retire copies verdicts on the fifth submit, in s2k_wait_all and
    in s2k_ctx_destroy): a Ticket that is dropped without wait() must not take its arrays with it.  A ticket
    leaves the table when it is waited for, or when the library has retired it: at most four are in flight, the submit of
    ticket t + 4 retires ticket t before it returns."""
    _IN_FLIGHT = 4

    def _hold(self, ticket: int, out, keep):
        if not hasattr(self, "_inflight"):
            self._inflight = {}
        self._inflight[ticket] = (out, keep)
        for t in [t for t in self._inflight if t + self._IN_FLIGHT <= ticket]:
            del self._inflight[t]
        return Ticket(self, ticket, out)

    def _release(self, ticket: int):
        getattr(self, "_inflight", {}).pop(ticket, None)


class Engine(_TicketOwner):
    """One context bound to one GPU (s2k_ctx)."""

    def __init__(self, device: int = 0, gt_bits: int = 0, wait_tables: bool = False):
        """gt_bits 0: automatic generator tables (usable at once on a narrow table, the wide one is built in the background);
        16..26: exactly that window width, built before the constructor returns.  wait_tables: return only when the
        background build has ended (s2k_ctx_create_ex)."""
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.s2k_ctx_create_ex(device, int(gt_bits), CTX_WAIT_TABLES if wait_tables else 0, C.byref(h))
        if rc != 0:
            raise EngineError(f"s2k_ctx_create failed ({rc}): {self._lib.s2k_last_error(None).decode()}")
        self._h = h
        self.device = device

    def gt_info(self) -> dict:
        """generator tables of this context's device: window bits in use now, bits the background build aims for, whether it
        is running, bytes held, and the reason for the choice (s2k_ctx_gt_info / s2k_ctx_gt_note)"""
        info = (C.c_uint64 * 4)()
        self._check(self._lib.s2k_ctx_gt_info(self._h, info))
        return {"bits": int(info[0]), "target_bits": int(info[1]), "building": bool(info[2]), "bytes": int(info[3]),
                "note": self._lib.s2k_ctx_gt_note(self._h).decode()}

    def debug_gt_swap_in_call(self, bits: int):
        """test hook (s2k_debug_gt_swap_in_call): the next ecdsa_verify_batch publishes the `bits`-wide generator table for the
        device's automatic contexts between its ladder launch and its worklist launch"""
        self._check(self._lib.s2k_debug_gt_swap_in_call(self._h, int(bits)))

    def set_small_batch_max(self, max_n: int):
        """batches of up to max_n signatures take the wave-per-signature ladder (s2k_ctx_set_small_batch_max; 0: never)"""
        self._check(self._lib.s2k_ctx_set_small_batch_max(self._h, int(max_n)))

    def set_mid_batch_max(self, max_n: int):
        """ECDSA batches above the small-batch threshold and up to max_n take the four-lanes-per-signature ladder (0: never)"""
        self._check(self._lib.s2k_ctx_set_mid_batch_max(self._h, int(max_n)))

    def gt_wait(self) -> int:
        """block until the background build of the wide generator tables has ended; the window bits in use then"""
        return int(self._lib.s2k_ctx_gt_wait(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.s2k_ctx_destroy(self._h)      # (retires the batches in flight: their buffers are needed until it returns)
            self._h = None
            self._inflight = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise EngineError(f"engine call failed ({rc}): {self._lib.s2k_last_error(self._h).decode()}")

    def _wait(self, ticket):
        self._check(self._lib.s2k_wait(self._h, ticket))

    def _poll(self, ticket) -> bool:
        rc = self._lib.s2k_poll(self._h, ticket)
        if rc == 1:          # S2K_PENDING
            return False
        self._check(rc)
        return True

    # ---- hot path -------------------------------------------------------------------
    def ecdsa_verify_batch(self, pub_xy, digest32, r, s, reject_malleable: bool = False,
                           force_complete: bool = False, force_worklist: bool = False) -> np.ndarray:
        """valid bits (uint8 0/1) for n (pubkey, digest, r, s) tuples; host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        pub_xy, digest32, s = _arr(pub_xy, 64, n), _arr(digest32, 32, n), _arr(s, 32, n)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_batch(self._h, n, pub_xy.ctypes.data, digest32.ctypes.data,
                                                     r.ctypes.data, s.ctypes.data,
                                                     (REJECT_MALLEABLE if reject_malleable else 0) |
                                                     (FORCE_COMPLETE if force_complete else 0) |
                                                     (FORCE_WORKLIST if force_worklist else 0), out.ctypes.data))
        return out

    # ---- submit / wait -------------------------------------------------------------------
    def ecdsa_verify_batch_submit(self, pub_xy, digest32, r, s, out=None, reject_malleable: bool = False) -> "Ticket":
        """s2k_ecdsa_verify_batch_submit: enqueue the batch and return; `Ticket.wait()` gives the valid bits.  The input
        arrays are used as they are (no copies: pass contiguous uint8 arrays of the right shapes, page-locked ones
        from pinned_array for asynchronous transfers) and are kept alive by the ticket."""
        arrs = []
        n = None
        for a, w in ((pub_xy, 64), (digest32, 32), (r, 32), (s, 32)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]):
                a = _arr(a, w)
            a = a.reshape(-1, w)
            if n is None:
                n = a.shape[0]
            elif a.shape[0] != n:
                raise ValueError(f"length mismatch: expected {n} items, got {a.shape[0]}")
            arrs.append(a)
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_ecdsa_verify_batch_submit(self._h, n, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                                            arrs[3].ctypes.data, REJECT_MALLEABLE if reject_malleable else 0,
                                                            out.ctypes.data, C.byref(t)))
        return self._hold(int(t.value), out, arrs)

    def ecdsa_verify_encoded_batch_submit(self, pubs, digests, sigs, encoding=ENCODING_ASN1, digest_len=0,
                                          reject_malleable=False, bip0066=False) -> "Ticket":
        """s2k_ecdsa_verify_encoded_batch_submit for lists of byte strings (or pre-built (blob, offsets) pairs)."""
        def cat(x):
            return x if isinstance(x, tuple) else _concat(list(x))
        (pb, po), (db, do), (sb, so) = cat(pubs), cat(digests), cat(sigs)
        n = len(po) - 1
        if len(do) - 1 != n or len(so) - 1 != n:
            raise ValueError("length mismatch")
        out = np.zeros(n, dtype=np.uint8)
        flags = (REJECT_MALLEABLE if reject_malleable else 0) | (BIP0066 if bip0066 else 0)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_ecdsa_verify_encoded_batch_submit(self._h, n, pb.ctypes.data, po.ctypes.data, db.ctypes.data,
                                                                    do.ctypes.data, sb.ctypes.data, so.ctypes.data, encoding,
                                                                    digest_len, flags, out.ctypes.data, C.byref(t)))
        return self._hold(int(t.value), out, [pb, po, db, do, sb, so])

    def wait_all(self):
        self._check(self._lib.s2k_wait_all(self._h))
        self._inflight = {}

    # ---- key sets ----------------------------------------------------------------------
    def keyset_create(self, pub_xy, layout: int = 0, capacity: int = 0) -> "KeySet":
        """Per-key tables of a list of public keys (n_keys x 64 bytes), built once (s2k_keyset_create_cap);
        layout: KEYSET_AUTO (0: the widest of JOINT5 and JOINT that fits, else CHUNKS), KEYSET_CHUNKS (1), KEYSET_JOINT (2),
        KEYSET_JOINT5 (3), KEYSET_JOINT6 (4) or KEYSET_COMB (5: 10 KiB per key, for long key lists); keyset_geometry().
        capacity: keys the set has memory for (0: as many as pub_xy holds); KeySet.append adds keys up to it."""
        return KeySet(self, pub_xy, layout, capacity)

    def ecdsa_verify_batch_keyset(self, keyset, key_index, digest32, r, s, reject_malleable: bool = False,
                                  force_worklist: bool = False) -> np.ndarray:
        """valid bits for n (key index into `keyset`, digest, r, s) tuples; host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        digest32, s = _arr(digest32, 32, n), _arr(s, 32, n)
        ki = np.ascontiguousarray(key_index, dtype=np.uint32).reshape(-1)
        if ki.shape[0] != n:
            raise ValueError(f"length mismatch: expected {n} key indices, got {ki.shape[0]}")
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_batch_keyset(self._h, keyset._k, n, ki.ctypes.data, digest32.ctypes.data,
                                                            r.ctypes.data, s.ctypes.data,
                                                            (REJECT_MALLEABLE if reject_malleable else 0) |
                                                            (FORCE_WORKLIST if force_worklist else 0), out.ctypes.data))
        return out

    def ecdsa_verify_batch_keyset_submit(self, keyset, key_index, digest32, r, s, out=None, reject_malleable: bool = False) -> "Ticket":
        """s2k_ecdsa_verify_batch_keyset_submit: as ecdsa_verify_batch_submit, the keys named by their index in `keyset`
        (contiguous arrays are used as they are - uint32 indices, uint8 rows - and kept alive by the ticket)."""
        ki = key_index if (isinstance(key_index, np.ndarray) and key_index.dtype == np.uint32 and key_index.flags["C_CONTIGUOUS"]) \
            else np.ascontiguousarray(key_index, dtype=np.uint32)
        ki = ki.reshape(-1)
        n = ki.shape[0]
        arrs = [ki]
        for a in (digest32, r, s):
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]):
                a = _arr(a, 32)
            a = a.reshape(-1, 32)
            if a.shape[0] != n:
                raise ValueError(f"length mismatch: expected {n} items, got {a.shape[0]}")
            arrs.append(a)
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_ecdsa_verify_batch_keyset_submit(self._h, keyset._k, n, arrs[0].ctypes.data, arrs[1].ctypes.data,
                                                                   arrs[2].ctypes.data, arrs[3].ctypes.data,
                                                                   REJECT_MALLEABLE if reject_malleable else 0, out.ctypes.data,
                                                                   C.byref(t)))
        return self._hold(int(t.value), out, arrs + [keyset])

    def ecdsa_verify_batch_keyset_device(self, keyset, n, d_key_index, d_digest32, d_r, d_s, d_valid, flags=0, stream=0):
        self._check(self._lib.s2k_ecdsa_verify_batch_keyset_device(self._h, keyset._k, int(n), d_key_index, d_digest32, d_r, d_s,
                                                                   int(flags), d_valid, stream))

    # ---- key sets by key bytes (the set needs an index: KeySet.index_create) ------------------
    def keyset_lookup(self, keyset, keys, key_bytes: int = 64, stride: int = 0, offset: int = 0) -> np.ndarray:
        """uint32 array: for every key the lowest index of a key of `keyset` with the same bytes (key_bytes 64: X || Y; 32:
        X), else 0xFFFFFFFF (s2k_keyset_lookup).  key_bytes 33: SEC1 compressed keys, answered with the index of the point
        they decode to (no square root is taken), 0xFFFFFFFF when they decode to nothing.  `keys`: n rows of key_bytes
        bytes; or, with `stride`, a buffer of records of `stride` bytes whose key begins `offset` bytes into each (65-byte
        SEC1 records: stride=65, offset=1)."""
        key_bytes = int(key_bytes)
        if key_bytes not in (32, 33, 64):
            raise ValueError("key_bytes is 64, 32 or 33")
        if stride:
            stride, offset = int(stride), int(offset)
            buf = _arr(keys, 1).reshape(-1)
            if stride < key_bytes or offset < 0 or offset + key_bytes > stride or buf.size % stride:
                raise ValueError(f"records of {stride} bytes with a {key_bytes}-byte key at offset {offset}: bad buffer of {buf.size} bytes")
            n = buf.size // stride
        else:
            buf, stride, offset = _arr(keys, key_bytes), key_bytes, 0
            n = buf.shape[0]
        out = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.s2k_keyset_lookup(self._h, keyset._k, n, buf.ctypes.data + offset if n else None, key_bytes, stride,
                                                out.ctypes.data))
        return out

    def keyset_lookup_device(self, keyset, n, d_keys, d_key_index, key_bytes: int = 64, stride: int = 0, stream=0):
        """Device-pointer form (s2k_keyset_lookup_device): n keys of key_bytes bytes at d_keys + i * stride (0: key_bytes),
        n uint32 indices to d_key_index; enqueued on `stream`."""
        self._check(self._lib.s2k_keyset_lookup_device(self._h, keyset._k, int(n), d_keys, int(key_bytes), int(stride) or int(key_bytes),
                                                       d_key_index, stream))

    def ecdsa_verify_batch_bykey(self, keyset, pub_xy, digest32, r, s, reject_malleable: bool = False,
                                 force_worklist: bool = False) -> np.ndarray:
        """ecdsa_verify_batch's verdicts for the same arrays, with the signatures whose key `keyset` holds verified on its
        tables and the others on the general ladder (s2k_ecdsa_verify_batch_keyset_bykey); host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        pub_xy, digest32, s = _arr(pub_xy, 64, n), _arr(digest32, 32, n), _arr(s, 32, n)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_batch_keyset_bykey(self._h, keyset._k, n, pub_xy.ctypes.data, digest32.ctypes.data,
                                                                  r.ctypes.data, s.ctypes.data,
                                                                  (REJECT_MALLEABLE if reject_malleable else 0) |
                                                                  (FORCE_WORKLIST if force_worklist else 0), out.ctypes.data))
        return out

    def ecdsa_verify_batch_bykey_device(self, keyset, n, d_pub_xy, d_digest32, d_r, d_s, d_valid, flags=0, stream=0):
        self._check(self._lib.s2k_ecdsa_verify_batch_keyset_bykey_device(self._h, keyset._k, int(n), d_pub_xy, d_digest32, d_r, d_s,
                                                                         int(flags), d_valid, stream))

    def ecdsa_verify_batch_bykey_submit(self, keyset, pub_xy, digest32, r, s, out=None, reject_malleable: bool = False) -> "Ticket":
        """s2k_ecdsa_verify_batch_keyset_bykey_submit: ecdsa_verify_batch_bykey as a ticket (contiguous uint8 arrays are used as
        they are and kept alive by the ticket, with the set)."""
        arrs = []
        for a, width in ((pub_xy, 64), (digest32, 32), (r, 32), (s, 32)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]):
                a = _arr(a, width)
            arrs.append(a.reshape(-1, width))
        n = arrs[2].shape[0]
        for a in arrs:
            if a.shape[0] != n:
                raise ValueError(f"length mismatch: expected {n} items, got {a.shape[0]}")
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_ecdsa_verify_batch_keyset_bykey_submit(self._h, keyset._k, n, arrs[0].ctypes.data, arrs[1].ctypes.data,
                                                                         arrs[2].ctypes.data, arrs[3].ctypes.data,
                                                                         REJECT_MALLEABLE if reject_malleable else 0, out.ctypes.data,
                                                                         C.byref(t)))
        return self._hold(int(t.value), out, arrs + [keyset])

    def ecdsa_verify_encoded_batch(self, pubs, digests, sigs, encoding=ENCODING_ASN1, digest_len=0,
                                   reject_malleable=False, bip0066=False, force_complete=False) -> np.ndarray:
        """PublicKey.Verify(digest, sig, opts) for lists of SEC1 keys, digests and encoded signatures (or pre-built
        (blob, offsets) pairs, as the submit form takes)."""
        def cat(x):
            return x if isinstance(x, tuple) else _concat(list(x))
        (pb, po), (db, do), (sb, so) = cat(pubs), cat(digests), cat(sigs)
        n = len(po) - 1
        if len(do) - 1 != n or len(so) - 1 != n:
            raise ValueError("length mismatch")
        out = np.zeros(n, dtype=np.uint8)
        flags = (REJECT_MALLEABLE if reject_malleable else 0) | (BIP0066 if bip0066 else 0) | \
                (FORCE_COMPLETE if force_complete else 0)
        self._check(self._lib.s2k_ecdsa_verify_encoded_batch(self._h, n, pb.ctypes.data, po.ctypes.data, db.ctypes.data,
                                                             do.ctypes.data, sb.ctypes.data, so.ctypes.data, encoding,
                                                             digest_len, flags, out.ctypes.data))
        return out

    def _encoded_keyset_args(self, pubs, digests, sigs, reject_malleable, bip0066, force_worklist):
        def cat(x):
            return x if isinstance(x, tuple) else _concat(list(x))
        (pb, po), (db, do), (sb, so) = cat(pubs), cat(digests), cat(sigs)
        n = len(po) - 1
        if len(do) - 1 != n or len(so) - 1 != n:
            raise ValueError("length mismatch")
        flags = (REJECT_MALLEABLE if reject_malleable else 0) | (BIP0066 if bip0066 else 0) | (FORCE_WORKLIST if force_worklist else 0)
        return n, [pb, po, db, do, sb, so], flags

    def ecdsa_verify_encoded_batch_keyset(self, keyset, pubs, digests, sigs, encoding=ENCODING_ASN1, digest_len=0,
                                          reject_malleable=False, bip0066=False, force_worklist=False) -> np.ndarray:
        """ecdsa_verify_encoded_batch's verdicts for the same arguments, with the signatures whose key `keyset` holds verified
        on its tables; a compressed key of the set costs no square root (s2k_ecdsa_verify_encoded_batch_keyset).  Lists of
        byte strings, or pre-built (blob, offsets) pairs."""
        n, a, flags = self._encoded_keyset_args(pubs, digests, sigs, reject_malleable, bip0066, force_worklist)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_encoded_batch_keyset(self._h, keyset._k, n, *(x.ctypes.data for x in a), int(encoding),
                                                                    int(digest_len), flags, out.ctypes.data))
        return out

    def ecdsa_verify_encoded_batch_keyset_submit(self, keyset, pubs, digests, sigs, encoding=ENCODING_ASN1, digest_len=0,
                                                 reject_malleable=False, bip0066=False, force_worklist=False) -> "Ticket":
        """s2k_ecdsa_verify_encoded_batch_keyset_submit: one ticket, the whole batch in one piece; the ticket keeps the
        buffers and the set alive."""
        n, a, flags = self._encoded_keyset_args(pubs, digests, sigs, reject_malleable, bip0066, force_worklist)
        out = np.zeros(n, dtype=np.uint8)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_ecdsa_verify_encoded_batch_keyset_submit(self._h, keyset._k, n, *(x.ctypes.data for x in a),
                                                                           int(encoding), int(digest_len), flags, out.ctypes.data,
                                                                           C.byref(t)))
        return self._hold(int(t.value), out, a + [keyset])

    def last_encoded_keyset_stats(self) -> dict:
        """of the last synchronous ecdsa_verify_encoded_batch_keyset, summed over its pieces: signatures verified under a key
        of the set that came as 33 / as 65 bytes, the length of the decompression list (= square roots taken), and the items
        of the pieces the set was not used for (s2k_ctx_last_encoded_keyset_stats)"""
        o = (C.c_uint64 * 4)()
        self._check(self._lib.s2k_ctx_last_encoded_keyset_stats(self._h, o))
        return {"hits33": int(o[0]), "hits65": int(o[1]), "roots": int(o[2]), "delegated": int(o[3])}

    def debug_parse_encoded(self, pubs, digests, sigs, first=0, cnt=None, encoding=ENCODING_ASN1, digest_len=0, reject_malleable=False,
                            bip0066=False, keyset=None, new_call=True, sentinel=0xA5) -> dict:
        """test hook (s2k_debug_parse_encoded): the parse step of the encoded calls for the piece [first, first + cnt) of the
        batch, no ladder.  Lists of byte strings or (blob, offsets) pairs.  Returns the arrays of the WHOLE batch - xy (n, 64),
        dg / r / s (n, 32), recid (n,) for the recoverable encoding - with `sentinel` in every byte the kernels did not write,
        and over a key set found (cnt,), the decompression list, and the call's counters after k_decompress_list ("before")
        and after k_decompress_list_close ("after") as dicts of hits33 / hits65 / roots / list."""
        n, a, flags = self._encoded_keyset_args(pubs, digests, sigs, reject_malleable, bip0066, False)
        cnt = n - first if cnt is None else cnt
        o = dict(xy=np.zeros((n, 64), np.uint8), dg=np.zeros((n, 32), np.uint8), r=np.zeros((n, 32), np.uint8), s=np.zeros((n, 32), np.uint8))
        recid = np.zeros(n, np.uint8) if encoding == ENCODING_COMPACT_RECOVERABLE else None
        found, lst, ctr = np.zeros(max(cnt, 1), np.uint32), np.zeros(max(cnt, 1), np.uint32), np.zeros(8, np.uint32)
        self._check(self._lib.s2k_debug_parse_encoded(self._h, keyset._k if keyset is not None else None, n, *(x.ctypes.data for x in a),
                                                      int(first), int(cnt), int(encoding), int(digest_len), flags, 1 if new_call else 0,
                                                      int(sentinel), o["xy"].ctypes.data, o["dg"].ctypes.data, o["r"].ctypes.data,
                                                      o["s"].ctypes.data, None if recid is None else recid.ctypes.data, found.ctypes.data,
                                                      lst.ctypes.data, ctr.ctypes.data))
        if recid is not None:
            o["recid"] = recid
        if keyset is not None:
            names = ("hits33", "hits65", "roots", "list")
            o["before"] = dict(zip(names, (int(v) for v in ctr[:4])))
            o["after"] = dict(zip(names, (int(v) for v in ctr[4:])))
            o["found"] = found[:cnt]
            o["list"] = lst[:o["before"]["list"]]
        return o

    def ecdsa_verify_batch_device(self, n, d_pub_xy, d_digest32, d_r, d_s, d_valid, flags=0, stream=0):
        """Device-pointer form: integer device addresses, enqueued on `stream` (a hipStream_t value)."""
        self._check(self._lib.s2k_ecdsa_verify_batch_device(self._h, int(n), d_pub_xy, d_digest32, d_r, d_s,
                                                            int(flags), d_valid, stream))

    # ---- SHA-2 digests on the device, and ECDSA verification from messages (digest.hip) ----------
    def digest_batch(self, msgs, alg: int = HASH_SHA256, out_len: int = 32, out_stride: int = 0, out=None) -> np.ndarray:
        """s2k_digest_batch: (n, out_len) digests of the messages (`msgs`: a list of byte strings, a (blob, offsets) pair or an
        (n, L) uint8 array); alg HASH_SHA256 / HASH_SHA256D / HASH_SHA512 / HASH_KECCAK256 / HASH_SHA3_256, out_len 32 or,
        with HASH_SHA512, 64.
        out_stride (test hook s2k_debug_digest_strided): rows that far apart in `out`, an (n, out_stride) uint8 array that
        goes to the device as it is and comes back with only the first out_len bytes of each row written."""
        n, blob, offs, mlen, keep = _messages(msgs)
        if out_stride:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.shape == (n, out_stride)):
                raise ValueError("out: a contiguous (n, out_stride) uint8 array is needed")
            self._check(self._lib.s2k_debug_digest_strided(self._h, int(alg), n, blob, offs, mlen, out.ctypes.data, int(out_len), int(out_stride)))
            return out
        res = np.zeros((n, int(out_len)), dtype=np.uint8)
        self._check(self._lib.s2k_digest_batch(self._h, int(alg), n, blob, offs, mlen, res.ctypes.data, int(out_len)))
        return res

    def digest_batch_device(self, alg, n, d_msgs, d_msg_offsets, msg_len, d_out, out_len=32, stream=0):
        self._check(self._lib.s2k_digest_batch_device(self._h, int(alg), int(n), d_msgs, d_msg_offsets, int(msg_len), d_out, int(out_len), stream))

    @staticmethod
    def _ecdsa_flags(reject_malleable, force_complete=False, force_worklist=False):
        return (REJECT_MALLEABLE if reject_malleable else 0) | (FORCE_COMPLETE if force_complete else 0) | (FORCE_WORKLIST if force_worklist else 0)

    def ecdsa_verify_messages_batch(self, pub_xy, msgs, r, s, alg: int = HASH_SHA256, reject_malleable: bool = False,
                                    force_complete: bool = False, force_worklist: bool = False) -> np.ndarray:
        """ecdsa_verify_batch on the digests of `msgs`, hashed on the device (s2k_ecdsa_verify_messages_batch); host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        pub_xy, s = _arr(pub_xy, 64, n), _arr(s, 32, n)
        _, blob, offs, mlen, keep = _messages(msgs, n)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_messages_batch(self._h, n, pub_xy.ctypes.data, int(alg), blob, offs, mlen, r.ctypes.data, s.ctypes.data,
                                                              self._ecdsa_flags(reject_malleable, force_complete, force_worklist), out.ctypes.data))
        return out

    def ecdsa_verify_messages_batch_submit(self, pub_xy, msgs, r, s, alg: int = HASH_SHA256, out=None, reject_malleable: bool = False) -> "Ticket":
        """s2k_ecdsa_verify_messages_batch_submit: as ecdsa_verify_batch_submit (contiguous uint8 arrays are used as they are;
        everything, the messages included, is kept alive by the ticket)."""
        arrs = []
        for a, w in ((pub_xy, 64), (r, 32), (s, 32)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]):
                a = _arr(a, w)
            arrs.append(a.reshape(-1, w))
        n = arrs[1].shape[0]
        if arrs[0].shape[0] != n or arrs[2].shape[0] != n:
            raise ValueError(f"length mismatch: expected {n} items")
        _, blob, offs, mlen, keep = _messages(msgs, n)
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_ecdsa_verify_messages_batch_submit(self._h, n, arrs[0].ctypes.data, int(alg), blob, offs, mlen, arrs[1].ctypes.data,
                                                                     arrs[2].ctypes.data, REJECT_MALLEABLE if reject_malleable else 0,
                                                                     out.ctypes.data, C.byref(t)))
        return self._hold(int(t.value), out, arrs + keep)

    def ecdsa_verify_messages_batch_device(self, n, d_pub_xy, alg, d_msgs, d_msg_offsets, msg_len, d_r, d_s, d_valid, flags=0, stream=0):
        """Device-pointer form (s2k_ecdsa_verify_messages_batch_device): d_msg_offsets None for n messages of msg_len bytes."""
        self._check(self._lib.s2k_ecdsa_verify_messages_batch_device(self._h, int(n), d_pub_xy, int(alg), d_msgs, d_msg_offsets, int(msg_len),
                                                                     d_r, d_s, int(flags), d_valid, stream))

    def ecdsa_verify_messages_batch_keyset(self, keyset, key_index, msgs, r, s, alg: int = HASH_SHA256, reject_malleable: bool = False,
                                           force_worklist: bool = False) -> np.ndarray:
        """ecdsa_verify_batch_keyset on the digests of `msgs`, hashed on the device; host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        s = _arr(s, 32, n)
        ki = np.ascontiguousarray(key_index, dtype=np.uint32).reshape(-1)
        if ki.shape[0] != n:
            raise ValueError(f"length mismatch: expected {n} key indices, got {ki.shape[0]}")
        _, blob, offs, mlen, keep = _messages(msgs, n)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_messages_batch_keyset(self._h, keyset._k, n, ki.ctypes.data, int(alg), blob, offs, mlen, r.ctypes.data,
                                                                     s.ctypes.data, self._ecdsa_flags(reject_malleable, False, force_worklist),
                                                                     out.ctypes.data))
        return out

    def ecdsa_verify_messages_batch_keyset_device(self, keyset, n, d_key_index, alg, d_msgs, d_msg_offsets, msg_len, d_r, d_s, d_valid, flags=0, stream=0):
        self._check(self._lib.s2k_ecdsa_verify_messages_batch_keyset_device(self._h, keyset._k, int(n), d_key_index, int(alg), d_msgs, d_msg_offsets,
                                                                            int(msg_len), d_r, d_s, int(flags), d_valid, stream))

    def ecdsa_verify_messages_batch_bykey(self, keyset, pub_xy, msgs, r, s, alg: int = HASH_SHA256, reject_malleable: bool = False,
                                          force_worklist: bool = False) -> np.ndarray:
        """ecdsa_verify_batch_bykey on the digests of `msgs`, hashed on the device; host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        pub_xy, s = _arr(pub_xy, 64, n), _arr(s, 32, n)
        _, blob, offs, mlen, keep = _messages(msgs, n)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_verify_messages_batch_keyset_bykey(self._h, keyset._k, n, pub_xy.ctypes.data, int(alg), blob, offs, mlen,
                                                                           r.ctypes.data, s.ctypes.data,
                                                                           self._ecdsa_flags(reject_malleable, False, force_worklist), out.ctypes.data))
        return out

    def ecdsa_verify_messages_batch_bykey_device(self, keyset, n, d_pub_xy, alg, d_msgs, d_msg_offsets, msg_len, d_r, d_s, d_valid, flags=0, stream=0):
        self._check(self._lib.s2k_ecdsa_verify_messages_batch_keyset_bykey_device(self._h, keyset._k, int(n), d_pub_xy, int(alg), d_msgs, d_msg_offsets,
                                                                                  int(msg_len), d_r, d_s, int(flags), d_valid, stream))

    def schnorr_verify_batch(self, pk32, msgs, sig64, force_complete: bool = False) -> np.ndarray:
        """BIP-340: valid bits for n (x-only key, message, 64-byte signature) triples.
        `msgs` is a list of byte strings (any lengths) or an (n, L) uint8 array."""
        pk32 = _arr(pk32, 32)
        n = pk32.shape[0]
        sig64 = _arr(sig64, 64, n)
        flags = FORCE_COMPLETE if force_complete else 0
        out = np.zeros(n, dtype=np.uint8)
        if isinstance(msgs, (list, tuple)):
            if len(msgs) != n:
                raise ValueError(f"length mismatch: expected {n} messages, got {len(msgs)}")
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            self._check(self._lib.s2k_schnorr_verify_batch(self._h, n, pk32.ctypes.data, blob.ctypes.data,
                                                           offs.ctypes.data, 0, sig64.ctypes.data, flags, out.ctypes.data))
        else:
            m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
            self._check(self._lib.s2k_schnorr_verify_batch(self._h, n, pk32.ctypes.data, m.ctypes.data if m.size else None,
                                                           None, m.shape[1], sig64.ctypes.data, flags, out.ctypes.data))
        return out

    def schnorr_verify_batch_keyset(self, keyset, key_index, msgs, sig64) -> np.ndarray:
        """BIP-340 over a key set (s2k_schnorr_verify_batch_keyset): signature i is verified under the x coordinate of key
        key_index[i] of `keyset` (a set of X || Y keys; the parity of Y does not matter)."""
        ki = np.ascontiguousarray(key_index, dtype=np.uint32).reshape(-1)
        n = ki.shape[0]
        sig64 = _arr(sig64, 64, n)
        out = np.zeros(n, dtype=np.uint8)
        if isinstance(msgs, (list, tuple)):
            if len(msgs) != n:
                raise ValueError(f"length mismatch: expected {n} messages, got {len(msgs)}")
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            self._check(self._lib.s2k_schnorr_verify_batch_keyset(self._h, keyset._k, n, ki.ctypes.data, blob.ctypes.data, offs.ctypes.data, 0,
                                                                  sig64.ctypes.data, 0, out.ctypes.data))
        else:
            m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
            self._check(self._lib.s2k_schnorr_verify_batch_keyset(self._h, keyset._k, n, ki.ctypes.data, m.ctypes.data if m.size else None, None,
                                                                  m.shape[1], sig64.ctypes.data, 0, out.ctypes.data))
        return out

    def schnorr_verify_batch_keyset_submit(self, keyset, key_index, msgs, sig64, out=None) -> "Ticket":
        """s2k_schnorr_verify_batch_keyset_submit; `msgs` an (n, L) uint8 array (fixed-length messages) or a list of byte strings."""
        ki = np.ascontiguousarray(key_index, dtype=np.uint32).reshape(-1)
        n = ki.shape[0]
        sig64 = sig64 if (isinstance(sig64, np.ndarray) and sig64.dtype == np.uint8 and sig64.flags["C_CONTIGUOUS"]) else _arr(sig64, 64, n)
        out = _out_array(out, n)
        t = C.c_uint64(0)
        if isinstance(msgs, (list, tuple)):
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            keep = [ki, blob, offs, sig64, keyset]
            self._check(self._lib.s2k_schnorr_verify_batch_keyset_submit(self._h, keyset._k, n, ki.ctypes.data, blob.ctypes.data, offs.ctypes.data, 0,
                                                                         sig64.ctypes.data, 0, out.ctypes.data, C.byref(t)))
        else:
            m = msgs if (isinstance(msgs, np.ndarray) and msgs.dtype == np.uint8 and msgs.flags["C_CONTIGUOUS"]) else np.ascontiguousarray(msgs, dtype=np.uint8)
            m = m.reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
            keep = [ki, m, sig64, keyset]
            self._check(self._lib.s2k_schnorr_verify_batch_keyset_submit(self._h, keyset._k, n, ki.ctypes.data, m.ctypes.data if m.size else None, None,
                                                                         m.shape[1], sig64.ctypes.data, 0, out.ctypes.data, C.byref(t)))
        return self._hold(int(t.value), out, keep)

    def schnorr_verify_batch_keyset_device(self, keyset, n, d_key_index, d_msgs, msg_len, d_sig, d_valid, stream=0):
        self._check(self._lib.s2k_schnorr_verify_batch_keyset_device(self._h, keyset._k, int(n), d_key_index, d_msgs, None, int(msg_len), d_sig, 0,
                                                                     d_valid, stream))

    # ---- BIP-340 over a key set by x-only key bytes (the set needs an index: KeySet.index_create) ----
    @staticmethod
    def _schnorr_msgs(msgs, n):
        """(message buffer or None, offsets or None, msg_len, arrays to keep alive) as the s2k_schnorr_* calls take them"""
        if isinstance(msgs, (list, tuple)):
            if len(msgs) != n:
                raise ValueError(f"length mismatch: expected {n} messages, got {len(msgs)}")
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            return blob.ctypes.data, offs.ctypes.data, 0, [blob, offs]
        m = msgs if (isinstance(msgs, np.ndarray) and msgs.dtype == np.uint8 and msgs.flags["C_CONTIGUOUS"]) else np.ascontiguousarray(msgs, dtype=np.uint8)
        m = m.reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
        return (m.ctypes.data if m.size else None), None, m.shape[1], [m]

    def schnorr_verify_batch_bykey(self, keyset, pk32, msgs, sig64) -> np.ndarray:
        """schnorr_verify_batch's verdicts for the same arrays, with the signatures whose x-only key `keyset` holds as a valid
        key (either parity of Y) verified on its tables and the others on the general ladder
        (s2k_schnorr_verify_batch_keyset_bykey); host buffers.  `msgs`: a list of byte strings or an (n, L) uint8 array."""
        pk32 = _arr(pk32, 32)
        n = pk32.shape[0]
        sig64 = _arr(sig64, 64, n)
        m, offs, mlen, _keep = self._schnorr_msgs(msgs, n)       # (_keep: the message arrays live until the call returns)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_schnorr_verify_batch_keyset_bykey(self._h, keyset._k, n, pk32.ctypes.data, m, offs, mlen,
                                                                    sig64.ctypes.data, 0, out.ctypes.data))
        return out

    def schnorr_verify_batch_bykey_device(self, keyset, n, d_pk, d_msgs, msg_len, d_sig, d_valid, d_msg_offsets=None, flags=0, stream=0):
        """Device-pointer form (s2k_schnorr_verify_batch_keyset_bykey_device): integer device addresses, enqueued on `stream`;
        messages of msg_len bytes each, or concatenated under d_msg_offsets (n + 1 uint64)."""
        self._check(self._lib.s2k_schnorr_verify_batch_keyset_bykey_device(self._h, keyset._k, int(n), d_pk, d_msgs, d_msg_offsets, int(msg_len),
                                                                           d_sig, int(flags), d_valid, stream))

    def schnorr_verify_batch_bykey_submit(self, keyset, pk32, msgs, sig64, out=None) -> "Ticket":
        """s2k_schnorr_verify_batch_keyset_bykey_submit: schnorr_verify_batch_bykey as a ticket (contiguous uint8 arrays are used
        as they are and kept alive by the ticket, with the set)."""
        pk32 = pk32 if (isinstance(pk32, np.ndarray) and pk32.dtype == np.uint8 and pk32.flags["C_CONTIGUOUS"]) else _arr(pk32, 32)
        pk32 = pk32.reshape(-1, 32)
        n = pk32.shape[0]
        sig64 = sig64 if (isinstance(sig64, np.ndarray) and sig64.dtype == np.uint8 and sig64.flags["C_CONTIGUOUS"]) else _arr(sig64, 64, n)
        if sig64.reshape(-1, 64).shape[0] != n:
            raise ValueError(f"length mismatch: expected {n} signatures, got {sig64.reshape(-1, 64).shape[0]}")
        m, offs, mlen, keep = self._schnorr_msgs(msgs, n)
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_schnorr_verify_batch_keyset_bykey_submit(self._h, keyset._k, n, pk32.ctypes.data, m, offs, mlen,
                                                                           sig64.ctypes.data, 0, out.ctypes.data, C.byref(t)))
        return self._hold(int(t.value), out, keep + [pk32, sig64, keyset])

    def schnorr_batch_verify_rlc(self, pk32, msgs, sig64, seed32: bytes | None = None) -> bool:
        """True iff every (key, message, signature) triple verifies — one MSM of n + 2K + 2 terms
        (K distinct keys: the coefficients of a key's signatures are summed first)."""
        pk32 = _arr(pk32, 32)
        n = pk32.shape[0]
        sig64 = _arr(sig64, 64, n)
        seed = np.frombuffer(seed32 if seed32 is not None else os.urandom(32), dtype=np.uint8)
        if seed.size != 32:
            raise ValueError("seed32 must be 32 bytes")
        res = C.c_int(0)
        if isinstance(msgs, (list, tuple)):
            if len(msgs) != n:
                raise ValueError(f"length mismatch: expected {n} messages, got {len(msgs)}")
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            self._check(self._lib.s2k_schnorr_batch_verify_rlc(self._h, n, pk32.ctypes.data, blob.ctypes.data,
                                                               offs.ctypes.data, 0, sig64.ctypes.data, seed.ctypes.data,
                                                               C.byref(res)))
        else:
            m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
            self._check(self._lib.s2k_schnorr_batch_verify_rlc(self._h, n, pk32.ctypes.data,
                                                               m.ctypes.data if m.size else None, None,
                                                               m.shape[1] if n else 0, sig64.ctypes.data,
                                                               seed.ctypes.data, C.byref(res)))
        return bool(res.value)

    def schnorr_verify_batch_auto(self, pk32, msgs, sig64, seed32: bytes | None = None, return_stats: bool = False):
        """Valid bits like schnorr_verify_batch, at the cost of the whole-batch check when (as usual)
        everything verifies: one random-linear-combination MSM first; if that rejects, the failing
        signatures are located by bisection on the kept terms (s2k_schnorr_verify_batch_bisect)."""
        pk32 = _arr(pk32, 32)
        n = pk32.shape[0]
        sig64 = _arr(sig64, 64, n)
        seed = np.frombuffer(seed32 if seed32 is not None else os.urandom(32), dtype=np.uint8)
        if seed.size != 32:
            raise ValueError("seed32 must be 32 bytes")
        out = np.zeros(n, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint32)
        if isinstance(msgs, (list, tuple)):
            if len(msgs) != n:
                raise ValueError(f"length mismatch: expected {n} messages, got {len(msgs)}")
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            self._check(self._lib.s2k_schnorr_verify_batch_bisect(self._h, n, pk32.ctypes.data, blob.ctypes.data, offs.ctypes.data,
                                                                  0, sig64.ctypes.data, seed.ctypes.data, out.ctypes.data,
                                                                  stats.ctypes.data))
        else:
            m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
            self._check(self._lib.s2k_schnorr_verify_batch_bisect(self._h, n, pk32.ctypes.data, m.ctypes.data if m.size else None,
                                                                  None, m.shape[1] if n else 0, sig64.ctypes.data,
                                                                  seed.ctypes.data, out.ctypes.data, stats.ctypes.data))
        if return_stats:
            return out, {"sub_combinations": int(stats[0]), "verified_one_by_one": int(stats[1]), "levels": int(stats[2]),
                         "abandoned": bool(stats[3])}
        return out

    # ---- recoverable ECDSA signatures: the whole batch as one multi-scalar multiplication ----
    @staticmethod
    def _recoverable_args(pub_xy, digest32, r, s, recovery_id, seed32):
        """The five input arrays as (n, 64 / 32 / 32 / 32) and (n,) uint8 and the 32 seed bytes; ValueError on a row
        width other than 64/32/32/32/1, on lengths that disagree and on a seed that is not 32 bytes."""
        for a, w in ((pub_xy, 64), (digest32, 32), (r, 32), (s, 32)):
            if isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[1] != w:
                raise ValueError(f"row width {a.shape[1]}, expected {w}")
        r = _arr(r, 32)
        n = r.shape[0]
        pub_xy, digest32, s = _arr(pub_xy, 64, n), _arr(digest32, 32, n), _arr(s, 32, n)
        rid = _arr(recovery_id, 1, n).reshape(-1)
        seed = np.frombuffer(bytes(seed32) if seed32 is not None else os.urandom(32), dtype=np.uint8)
        if seed.size != 32:
            raise ValueError("seed32 must be 32 bytes")
        return n, pub_xy, digest32, r, s, rid, seed

    def ecdsa_batch_verify_rlc(self, pub_xy, digest32, r, s, recovery_id, seed32: bytes | None = None,
                               reject_malleable: bool = False) -> bool:
        """True iff for every item RecoverPublicKey(digest, r, s, recovery_id) is exactly the supplied key - one MSM of
        n + 2K + 2 terms for K distinct keys (s2k_ecdsa_batch_verify_rlc)."""
        n, pub_xy, digest32, r, s, rid, seed = self._recoverable_args(pub_xy, digest32, r, s, recovery_id, seed32)
        res = C.c_int(0)
        self._check(self._lib.s2k_ecdsa_batch_verify_rlc(self._h, n, pub_xy.ctypes.data, digest32.ctypes.data, r.ctypes.data,
                                                         s.ctypes.data, rid.ctypes.data, REJECT_MALLEABLE if reject_malleable else 0,
                                                         seed.ctypes.data, C.byref(res)))
        return bool(res.value)

    def ecdsa_verify_recoverable_batch(self, pub_xy, digest32, r, s, recovery_id, seed32: bytes | None = None,
                                       reject_malleable: bool = False, return_stats: bool = False):
        """Per-item verdicts (uint8 0/1) of the same contract at the price of the whole-batch check when everything is
        good; a rejected batch is bisected (s2k_ecdsa_verify_recoverable_batch_bisect)."""
        n, pub_xy, digest32, r, s, rid, seed = self._recoverable_args(pub_xy, digest32, r, s, recovery_id, seed32)
        out = np.zeros(n, dtype=np.uint8)
        stats = np.zeros(4, dtype=np.uint32)
        self._check(self._lib.s2k_ecdsa_verify_recoverable_batch_bisect(self._h, n, pub_xy.ctypes.data, digest32.ctypes.data,
                                                                        r.ctypes.data, s.ctypes.data, rid.ctypes.data,
                                                                        REJECT_MALLEABLE if reject_malleable else 0,
                                                                        seed.ctypes.data, out.ctypes.data, stats.ctypes.data))
        if return_stats:
            return out, {"sub_combinations": int(stats[0]), "verified_one_by_one": int(stats[1]), "levels": int(stats[2]),
                         "abandoned": bool(stats[3])}
        return out

    def ecdsa_batch_verify_rlc_device(self, n, d_pub_xy, d_digest32, d_r, d_s, d_recovery_id, seed32: bytes | None = None,
                                      flags=0, stream=0) -> bool:
        """Device-pointer form (integer device addresses; synchronises `stream` for the verdict)."""
        seed = np.frombuffer(bytes(seed32) if seed32 is not None else os.urandom(32), dtype=np.uint8)
        if seed.size != 32:
            raise ValueError("seed32 must be 32 bytes")
        res = C.c_int(0)
        self._check(self._lib.s2k_ecdsa_batch_verify_rlc_device(self._h, int(n), d_pub_xy, d_digest32, d_r, d_s, d_recovery_id,
                                                                int(flags), seed.ctypes.data, C.byref(res), stream))
        return bool(res.value)

    def ecdsa_verify_recoverable_batch_device(self, n, d_pub_xy, d_digest32, d_r, d_s, d_recovery_id, d_valid,
                                              seed32: bytes | None = None, flags=0, stream=0, return_stats: bool = False):
        """Device-pointer form of ecdsa_verify_recoverable_batch: the verdicts go to d_valid (n bytes), enqueued on `stream`."""
        seed = np.frombuffer(bytes(seed32) if seed32 is not None else os.urandom(32), dtype=np.uint8)
        if seed.size != 32:
            raise ValueError("seed32 must be 32 bytes")
        stats = np.zeros(4, dtype=np.uint32)
        self._check(self._lib.s2k_ecdsa_verify_recoverable_batch_bisect_device(self._h, int(n), d_pub_xy, d_digest32, d_r, d_s,
                                                                               d_recovery_id, int(flags), seed.ctypes.data, d_valid,
                                                                               stats.ctypes.data, stream))
        if return_stats:
            return {"sub_combinations": int(stats[0]), "verified_one_by_one": int(stats[1]), "levels": int(stats[2]),
                    "abandoned": bool(stats[3])}

    def ecdsa_recover_batch(self, digest32, r, s, recovery_id, force_complete: bool = False):
        """RecoverPublicKey over a batch: returns (pub65 (n,65) uint8, ok (n,) uint8)."""
        r = _arr(r, 32)
        n = r.shape[0]
        digest32, s = _arr(digest32, 32, n), _arr(s, 32, n)
        rid = np.ascontiguousarray(recovery_id, dtype=np.uint8).reshape(-1)
        if rid.shape[0] != n:
            raise ValueError("length mismatch")
        pub, ok = np.zeros((n, 65), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_recover_batch(self._h, n, digest32.ctypes.data, r.ctypes.data, s.ctypes.data,
                                                      rid.ctypes.data, FORCE_COMPLETE if force_complete else 0,
                                                      pub.ctypes.data, ok.ctypes.data))
        return pub, ok

    # ---- Keccak-256 addresses: of key records, and of recovered keys (address.hip) ----------
    def keccak_address_batch(self, pub65, ok=None) -> np.ndarray:
        """s2k_keccak_address_batch: (n, 20) addresses Keccak-256(X || Y)[12:] of the 65-byte records; 20 zero bytes for a
        record whose first byte is not 0x04 or whose ok (an optional (n,) uint8 array) is 0."""
        pub65 = _arr(pub65, 65)
        n = pub65.shape[0]
        okp = None
        if ok is not None:
            ok = np.ascontiguousarray(ok, dtype=np.uint8).reshape(-1)
            if ok.shape[0] != n:
                raise ValueError("length mismatch")
            okp = ok.ctypes.data
        addr = np.zeros((n, 20), dtype=np.uint8)
        self._check(self._lib.s2k_keccak_address_batch(self._h, n, pub65.ctypes.data, okp, addr.ctypes.data))
        return addr

    def keccak_address_batch_device(self, n, d_pub65, d_ok, d_addr20, stream=0):
        """Device-pointer form: integer device addresses (d_ok None: every record counts), enqueued on `stream`."""
        self._check(self._lib.s2k_keccak_address_batch_device(self._h, int(n), d_pub65, d_ok, d_addr20, stream))

    def ecdsa_recover_address_batch(self, digest32, r, s, recovery_id, force_complete: bool = False):
        """ecdsa_recover_batch, then the address of each recovered key: returns (addr20 (n,20) uint8, ok (n,) uint8);
        20 zero bytes where ok is 0."""
        r = _arr(r, 32)
        n = r.shape[0]
        digest32, s = _arr(digest32, 32, n), _arr(s, 32, n)
        rid = np.ascontiguousarray(recovery_id, dtype=np.uint8).reshape(-1)
        if rid.shape[0] != n:
            raise ValueError("length mismatch")
        addr, ok = np.zeros((n, 20), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_recover_address_batch(self._h, n, digest32.ctypes.data, r.ctypes.data, s.ctypes.data,
                                                              rid.ctypes.data, FORCE_COMPLETE if force_complete else 0,
                                                              addr.ctypes.data, ok.ctypes.data))
        return addr, ok

    def ecdsa_recover_address_batch_device(self, n, d_digest32, d_r, d_s, d_recovery_id, d_addr20, d_ok, flags=0, stream=0):
        self._check(self._lib.s2k_ecdsa_recover_address_batch_device(self._h, int(n), d_digest32, d_r, d_s, d_recovery_id, int(flags),
                                                                     d_addr20, d_ok, stream))

    def ecdsa_recover_address_messages_batch(self, msgs, r, s, recovery_id, alg: int = HASH_KECCAK256, force_complete: bool = False):
        """ecdsa_recover_address_batch on the digests of `msgs`, hashed on the device with `alg`; host buffers."""
        r = _arr(r, 32)
        n = r.shape[0]
        s = _arr(s, 32, n)
        rid = np.ascontiguousarray(recovery_id, dtype=np.uint8).reshape(-1)
        if rid.shape[0] != n:
            raise ValueError("length mismatch")
        _, blob, offs, mlen, keep = _messages(msgs, n)
        addr, ok = np.zeros((n, 20), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_ecdsa_recover_address_messages_batch(self._h, n, int(alg), blob, offs, mlen, r.ctypes.data, s.ctypes.data,
                                                                       rid.ctypes.data, FORCE_COMPLETE if force_complete else 0,
                                                                       addr.ctypes.data, ok.ctypes.data))
        return addr, ok

    def ecdsa_recover_address_messages_batch_device(self, n, alg, d_msgs, d_msg_offsets, msg_len, d_r, d_s, d_recovery_id, d_addr20, d_ok,
                                                    flags=0, stream=0):
        """Device-pointer form: d_msg_offsets None for n messages of msg_len bytes."""
        self._check(self._lib.s2k_ecdsa_recover_address_messages_batch_device(self._h, int(n), int(alg), d_msgs, d_msg_offsets, int(msg_len),
                                                                              d_r, d_s, d_recovery_id, int(flags), d_addr20, d_ok, stream))

    def pack_valid_device(self, n, d_valid, d_bitmap, d_count, stream=0):
        """valid bytes -> bitmap + uint64 count, all device pointers."""
        self._check(self._lib.s2k_pack_valid_device(self._h, int(n), d_valid, d_bitmap, d_count, stream))

    def profile(self, enable: bool = True):
        """Per-kernel HIP-event timing of ecdsa_verify_batch_device calls (s2k_ctx_profile)."""
        self._check(self._lib.s2k_ctx_profile(self._h, 1 if enable else 0))

    def profile_read(self, cap: int = 1024):
        """-> dict(calls, prep_ms, fast_ms, fallback_ms (sums), fast_each (ms per call), shader_mhz = mean of
        the clock seen by the first wave and by a wave of the final round of the last ladder launch)."""
        sums = (C.c_double * 3)()
        each = (C.c_double * cap)()
        calls, mhz = C.c_size_t(0), (C.c_double * 2)()
        self._check(self._lib.s2k_ctx_profile_read(self._h, sums, each, cap, C.byref(calls), mhz))
        k = int(calls.value)
        both = [m for m in (mhz[0], mhz[1]) if m > 0]
        return {"calls": k, "prep_ms": sums[0], "fast_ms": sums[1], "fallback_ms": sums[2],
                "fast_each": [each[i] for i in range(min(k, cap))], "shader_mhz": sum(both) / len(both) if both else 0.0,
                "shader_mhz_first_wave": float(mhz[0]), "shader_mhz_last_round": float(mhz[1])}

    def profile_read_stages(self, cap: int = 1024):
        """-> dict(calls, prep_ms, group_ms (grouping by key + per-key tables), fast_ms (ladder over the per-key
        tables; the general ladder when grouping is off), left_ms (general ladder over the ungrouped rest),
        fallback_ms: sums; fast_each; shader_mhz...) (s2k_ctx_profile_read_stages)."""
        sums = (C.c_double * 5)()
        each = (C.c_double * cap)()
        calls, mhz = C.c_size_t(0), (C.c_double * 2)()
        self._check(self._lib.s2k_ctx_profile_read_stages(self._h, sums, each, cap, C.byref(calls), mhz))
        k = int(calls.value)
        both = [m for m in (mhz[0], mhz[1]) if m > 0]
        return {"calls": k, "prep_ms": sums[0], "group_ms": sums[1], "fast_ms": sums[2], "left_ms": sums[3],
                "fallback_ms": sums[4], "fast_each": [each[i] for i in range(min(k, cap))],
                "shader_mhz": sum(both) / len(both) if both else 0.0,
                "shader_mhz_first_wave": float(mhz[0]), "shader_mhz_last_round": float(mhz[1])}

    def profile_msm(self, enable: bool = True):
        """Stage timing of the multi-scalar path (s2k_ctx_profile_msm)."""
        self._check(self._lib.s2k_ctx_profile_msm(self._h, 1 if enable else 0))

    def profile_read_msm(self):
        """-> dict(calls, front_ms, sort_ms, bucket_pass_ms, reduce_ms, tail_ms): sums over the calls since the last read."""
        sums = (C.c_double * 5)()
        calls = C.c_size_t(0)
        self._check(self._lib.s2k_ctx_profile_read_msm(self._h, sums, C.byref(calls)))
        return {"calls": int(calls.value), "front_ms": sums[0], "sort_ms": sums[1], "bucket_pass_ms": sums[2],
                "reduce_ms": sums[3], "tail_ms": sums[4]}

    def set_key_grouping(self, mode: int = KEYS_AUTO, min_group: int = 0, hash_bits: int = 0, max_tables: int = 0):
        """How ecdsa_verify_batch[_device] treats signatures that share a public key (s2k_ctx_set_key_grouping):
        KEYS_OFF = every signature through the general kernel, KEYS_AUTO = keys with at least `min_group` (default 4, the
        measured break-even) signatures in the batch get a per-key table, KEYS_ALWAYS = every key does, KEYS_ADAPTIVE (what a
        new engine starts with) = KEYS_AUTO that stops looking for repeated keys after two large batches without any and looks
        again every sixteenth batch (key_grouping_adaptive)."""
        self._check(self._lib.s2k_ctx_set_key_grouping(self._h, int(mode), int(min_group), int(hash_bits), int(max_tables)))

    def set_keyed_ladder(self, ladder: int = LADDER_COMB):
        """Tables and ladder of the repeated keys of an ECDSA or BIP-340 call (s2k_ctx_set_keyed_ladder): LADDER_COMB (what a new engine
        starts with: 38 additions and 18 doublings per signature) or LADDER_WINDOW (16-bit chunks: 64 and 12)."""
        self._check(self._lib.s2k_ctx_set_keyed_ladder(self._h, int(ladder)))

    def set_keyset_small_batch_max(self, max_n: int):
        """key-set calls of up to max_n signatures take the wave-per-signature ladder over the set's tables
        (s2k_ctx_set_keyset_small_batch_max; 0: never; comb sets: set_keyset_comb_small_batch_max)"""
        self._check(self._lib.s2k_ctx_set_keyset_small_batch_max(self._h, int(max_n)))

    def set_keyset_comb_small_batch_max(self, max_n: int):
        """by-index calls over a KEYSET_COMB set of up to max_n signatures take the wave-per-signature ladder over the set's comb
        tables (s2k_ctx_set_keyset_comb_small_batch_max; 0, what a new engine starts with: never)"""
        self._check(self._lib.s2k_ctx_set_keyset_comb_small_batch_max(self._h, int(max_n)))

    def last_keyset_ladder(self) -> int:
        """KEYSET_LADDER_LANE / KEYSET_LADDER_ROW / KEYSET_LADDER_ROW_COMB: what the last key-set verification call enqueued; -1 before any."""
        return int(self._lib.s2k_ctx_last_keyset_ladder(self._h))

    def last_keyed_ladder(self) -> int:
        """LADDER_COMB / LADDER_WINDOW: the tables the last ECDSA or BIP-340 verification call built; -1: it built none."""
        return int(self._lib.s2k_ctx_last_keyed_ladder(self._h))

    def key_grouping_stats(self):
        """Of the last ecdsa_verify_batch_device call -> dict(keyed, tables, general, complete)."""
        st = (C.c_uint32 * 4)()
        self._check(self._lib.s2k_ctx_key_grouping_stats(self._h, st))
        return {"keyed": int(st[0]), "tables": int(st[1]), "general": int(st[2]), "complete": int(st[3])}

    def key_grouping_adaptive(self, reset: bool = False):
        """State of KEYS_ADAPTIVE, without synchronising -> dict(miss_streak, skip_left, skipped, probes, observed)."""
        st = (C.c_uint32 * 5)()
        self._check(self._lib.s2k_ctx_key_grouping_adaptive(self._h, st, 1 if reset else 0))
        return {"miss_streak": int(st[0]), "skip_left": int(st[1]), "skipped": int(st[2]), "probes": int(st[3]),
                "observed": int(st[4])}

    def workspace_bytes(self, n):
        return self._lib.s2k_ecdsa_workspace_bytes(int(n))

    def device_bytes(self, n):
        """Device memory this engine holds after a verification call of n signatures with the current grouping settings
        (generator tables + per-signature workspace + grouping arrays and per-key table buffer)."""
        return self._lib.s2k_ctx_device_bytes(self._h, int(n))

    # ---- group ----------------------------------------------------------------------
    def _points_out(self, n):
        return np.zeros((n, 65), dtype=np.uint8)

    def scalar_base_mult_batch(self, k):
        k = _arr(k, 32)
        out = self._points_out(k.shape[0])
        self._check(self._lib.s2k_scalar_base_mult_batch(self._h, k.shape[0], k.ctypes.data, out.ctypes.data))
        return out

    def scalar_mult_batch(self, k, points):
        k = _arr(k, 32)
        n = k.shape[0]
        points = _arr(points, 65, n)
        out = self._points_out(n)
        self._check(self._lib.s2k_scalar_mult_batch(self._h, n, k.ctypes.data, points.ctypes.data, out.ctypes.data))
        return out

    def double_scalar_mult_basepoint_batch(self, u1, u2, points):
        u1 = _arr(u1, 32)
        n = u1.shape[0]
        u2, points = _arr(u2, 32, n), _arr(points, 65, n)
        out = self._points_out(n)
        self._check(self._lib.s2k_double_scalar_mult_basepoint_batch(self._h, n, u1.ctypes.data, u2.ctypes.data,
                                                                     points.ctypes.data, out.ctypes.data))
        return out

    def double_scalar_mult_basepoint_batch_ex(self, impl, u1, u2, points):
        """u1*G + u2*P (u1 None: u2*P) with an implementation selector (IMPL_COMPLETE / IMPL_FAST)."""
        u2 = _arr(u2, 32)
        n = u2.shape[0]
        points = _arr(points, 65, n)
        u1a = _arr(u1, 32, n) if u1 is not None else None
        out = self._points_out(n)
        self._check(self._lib.s2k_double_scalar_mult_basepoint_batch_ex(self._h, impl, n,
                                                                        u1a.ctypes.data if u1a is not None else None,
                                                                        u2.ctypes.data, points.ctypes.data, out.ctypes.data))
        return out

    def fp_op_batch_ex(self, op, operands, lazy=0):
        """Hot-path field / group arithmetic (s2k_fp_op_batch_ex, IMPL_FAST): `operands` is a list of up
        to five (n,32) operand arrays (None = unused); returns (out, out2, flag)."""
        ops = [(_arr(x, 32) if x is not None else None) for x in operands] + [None] * (5 - len(operands))
        n = ops[0].shape[0]
        ptrs = (C.c_void_p * 5)(*[(x.ctypes.data if x is not None else None) for x in ops])
        out, out2, flag = (np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8))
        self._check(self._lib.s2k_fp_op_batch_ex(self._h, IMPL_FAST, op, lazy, n, ptrs, out.ctypes.data, out2.ctypes.data,
                                                 flag.ctypes.data))
        return out, out2, flag

    def fp_op_batch_ex8(self, op, operands, lazy=0, reps=0):
        """The same for operations of up to eight operands (s2k_fp_op_batch_ex8: HP_JADD_PAIR, the comb ladder's column);
        `lazy` holds operand j's code in bits 4j .. 4j + 3, `reps` chains the operation; returns (out, out2, flag)."""
        ops = [(_arr(x, 32) if x is not None else None) for x in operands] + [None] * (8 - len(operands))
        n = ops[0].shape[0]
        ptrs = (C.c_void_p * 8)(*[(x.ctypes.data if x is not None else None) for x in ops])
        out, out2, flag = (np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8))
        self._check(self._lib.s2k_fp_op_batch_ex8(self._h, IMPL_FAST, op, lazy, reps, n, ptrs, out.ctypes.data, out2.ctypes.data,
                                                  flag.ctypes.data))
        return out, out2, flag

    def fn_split_glv_odd_batch(self, k):
        """sc_split_glv_odd: (|k1|, |k2|, signs) with both magnitudes odd and below 2^129."""
        k = _arr(k, 32)
        n = k.shape[0]
        k1, k2, sg = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        self._check(self._lib.s2k_fn_split_glv_batch_ex(self._h, IMPL_FAST, n, k.ctypes.data, k1.ctypes.data, k2.ctypes.data,
                                                        sg.ctypes.data))
        return k1, k2, sg

    def point_add_batch(self, a, b):
        a = _arr(a, 65)
        n = a.shape[0]
        b = _arr(b, 65, n)
        out = self._points_out(n)
        self._check(self._lib.s2k_point_add_batch(self._h, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
        return out

    def point_double_batch(self, a):
        a = _arr(a, 65)
        out = self._points_out(a.shape[0])
        self._check(self._lib.s2k_point_double_batch(self._h, a.shape[0], a.ctypes.data, out.ctypes.data))
        return out

    def multi_scalar_mult(self, scalars, points) -> bytes:
        """sum_i scalars[i] * points[i] as a 65-byte record (MultiScalarMultVartime)."""
        scalars = _arr(scalars, 32)
        n = scalars.shape[0]
        points = _arr(points, 65, n)            # length mismatch raises, like the reference panics
        out = np.zeros(65, dtype=np.uint8)
        self._check(self._lib.s2k_multi_scalar_mult(self._h, n, scalars.ctypes.data if n else None,
                                                    points.ctypes.data if n else None, out.ctypes.data))
        return out.tobytes()

    def debug_msm_terms(self, mags, points, signs=None, window_bits=0, dump=False) -> dict:
        """test hook (s2k_debug_msm_terms): the multiscalar core on given terms - mags (n, 16) big-endian magnitudes, points
        (n, 65) records (all zero: an identity term), signs (n,) non-zero negates, window_bits 0 / 8 / 12 / 16.  Returns out
        (65 bytes), the geometry c / nw / nb / nslot / nkeys / L_A / nlanes / fold16, big (k_msm_stitch's counter of oversized
        buckets) and list_len; with dump the sort's offset[0 .. nkeys] and list[0 .. list_len) as well."""
        mags = _arr(mags, 16)
        n = mags.shape[0]
        points = _arr(points, 65, n)
        if signs is not None:
            signs = np.ascontiguousarray(signs, dtype=np.uint8).reshape(n)
        out, geom = np.zeros(65, dtype=np.uint8), np.zeros(10, dtype=np.uint32)
        offsets = np.zeros(9 * 32768 + 1, dtype=np.uint32) if dump else None          # (the largest key range: 16-bit windows)
        lst = np.zeros(max(16 * n, 1), dtype=np.uint32) if dump else None             # (at most 16 windows per term)
        self._check(self._lib.s2k_debug_msm_terms(self._h, n, mags.ctypes.data, points.ctypes.data,
                                                  None if signs is None else signs.ctypes.data, int(window_bits), out.ctypes.data,
                                                  geom.ctypes.data, None if offsets is None else offsets.ctypes.data,
                                                  0 if offsets is None else offsets.size, None if lst is None else lst.ctypes.data,
                                                  0 if lst is None else lst.size))
        o = dict(zip(("c", "nw", "nb", "nslot", "nkeys", "L_A", "nlanes", "fold16", "big", "list_len"), (int(v) for v in geom)))
        o["out"] = out.tobytes()
        if dump:
            o["offset"], o["list"] = offsets[:o["nkeys"] + 1], lst[:o["list_len"]]
        return o

    def _debug_rlc_result(self, n, call, key32, form, lo, cnt):
        key = np.frombuffer(bytes(key32), dtype=np.uint8)
        if key.size != 32:
            raise ValueError("key32 must be 32 bytes")
        out, status, in_comb = np.zeros(65, dtype=np.uint8), C.c_uint32(0), np.zeros(max(n, 1), dtype=np.uint8)
        self._check(call(key.ctypes.data, int(form), int(lo), int(n - lo if cnt is None else cnt), out.ctypes.data, C.byref(status),
                         in_comb.ctypes.data))
        return {"out": out.tobytes(), "status": int(status.value), "in_comb": in_comb[:n]}

    def debug_schnorr_rlc_point(self, pk32, msgs, sig64, key32: bytes, form: int = 0, lo: int = 0, cnt: int | None = None) -> dict:
        """test hook (s2k_debug_schnorr_rlc_point): the error point of a BIP-340 batch under the coefficient key `key32`, taken
        as given - form 0: the aggregated form of the whole batch, form 1: the plain form's sub-range [lo, lo + cnt) (cnt None:
        to the end).  Returns out (65 bytes: the affine record, zero for the identity), status (the device status word) and
        in_comb (n flags: the item took part in the sum).  `msgs`: a list of byte strings or an (n, L) uint8 array."""
        pk32 = _arr(pk32, 32)
        n = pk32.shape[0]
        sig64 = _arr(sig64, 64, n)
        m, offs, mlen, _keep = self._schnorr_msgs(msgs, n)       # (_keep: the message arrays live until the call returns)
        return self._debug_rlc_result(n, lambda *rest: self._lib.s2k_debug_schnorr_rlc_point(
            self._h, n, pk32.ctypes.data, m, offs, mlen, sig64.ctypes.data, *rest), key32, form, lo, cnt)

    def debug_ecdsa_rlc_point(self, pub_xy, digest32, r, s, recovery_id, key32: bytes, form: int = 0, lo: int = 0,
                              cnt: int | None = None, reject_malleable: bool = False) -> dict:
        """test hook (s2k_debug_ecdsa_rlc_point): the same for a batch of recoverable ECDSA signatures"""
        n, pub_xy, digest32, r, s, rid, _ = self._recoverable_args(pub_xy, digest32, r, s, recovery_id, bytes(32))
        return self._debug_rlc_result(n, lambda *rest: self._lib.s2k_debug_ecdsa_rlc_point(
            self._h, n, pub_xy.ctypes.data, digest32.ctypes.data, r.ctypes.data, s.ctypes.data, rid.ctypes.data,
            REJECT_MALLEABLE if reject_malleable else 0, *rest), key32, form, lo, cnt)

    def multi_scalar_mult_device(self, n, d_scalars, d_points, d_out65, stream=0):
        self._check(self._lib.s2k_multi_scalar_mult_device(self._h, int(n), d_scalars, d_points, d_out65, stream))

    def pointset_create(self, points, window_bits: int = 0) -> "PointSet":
        """Tables of a fixed list of points (m x 65-byte records), built once (s2k_pointset_create): segmented sums then name
        their points by index.  window_bits: 4, 8 or 0 (automatic).  Call .close() (or let it be collected) before the engine."""
        return PointSet(self, points, window_bits)

    def multi_scalar_mult_segments(self, scalars, points, offsets) -> np.ndarray:
        """out[j] = sum of scalars[i] * points[i] over offsets[j] <= i < offsets[j + 1] (MultiScalarMultVartime per segment):
        (n_seg, 65) records, an empty segment gives the identity record.  Public scalars only."""
        scalars = _arr(scalars, 32)
        n = scalars.shape[0]
        points = _arr(points, 65, n)            # length mismatch raises, like the reference panics
        off = check_segment_offsets(offsets, n)
        n_seg = off.shape[0] - 1
        out = np.zeros((n_seg, 65), dtype=np.uint8)
        self._check(self._lib.s2k_multi_scalar_mult_segments(self._h, n, scalars.ctypes.data if n else None,
                                                             points.ctypes.data if n else None, n_seg, off.ctypes.data,
                                                             out.ctypes.data if n_seg else None))
        return out

    def multi_scalar_mult_segments_device(self, n, d_scalars, d_points, offsets, d_out, stream=0):
        """The same on device buffers (d_out: n_seg * 65 bytes); `offsets` stays host memory.  Synchronises `stream` once."""
        off = check_segment_offsets(offsets, int(n))
        self._check(self._lib.s2k_multi_scalar_mult_segments_device(self._h, int(n), d_scalars, d_points, off.shape[0] - 1,
                                                                    off.ctypes.data, d_out, stream))

    # ---- hashing to the curve (RFC 9380; h2c.hip) -------------------------------------
    def expand_message_xmd(self, msgs, dst, len_in_bytes: int) -> np.ndarray:
        """expand_message_xmd with SHA-256 for every message (s2k_expand_message_xmd_batch): (n, len_in_bytes) uniform bytes.
        `msgs`: a list of byte strings or a (blob, offsets) pair; `dst`: the domain separation tag, common to the call."""
        dst, len_in_bytes = _h2c_dst(dst), int(len_in_bytes)
        if not 1 <= len_in_bytes <= 8160:
            raise ValueError("secp256k1/secec/h2c: len_in_bytes out of range")
        n, blob, offs = _h2c_messages(msgs)
        out = np.zeros((n, len_in_bytes), dtype=np.uint8)
        self._check(self._lib.s2k_expand_message_xmd_batch(self._h, n, dst, len(dst), blob.ctypes.data, offs.ctypes.data, 0,
                                                           len_in_bytes, out.ctypes.data if n else None))
        return out

    def map_to_curve(self, uniform, length: int, count: int = 1) -> np.ndarray:
        """out[i] = sum of `count` (1 or 2) points Point.SetUniformBytes(uniform[(i * count + j) * length ...]), 32 <= length
        <= 64 (s2k_map_to_curve_batch): (n, 65) records.  `uniform`: bytes, a list of byte strings or an array, n * count *
        length bytes in all."""
        length, count = int(length), int(count)
        if count not in (1, 2):
            raise ValueError("count must be 1 or 2")
        if not 32 <= length <= 64:
            raise ValueError("secp256k1: uniform bytes must be 32 to 64 bytes long")
        u = _arr(uniform, count * length)
        n = u.shape[0]
        out = self._points_out(n)
        self._check(self._lib.s2k_map_to_curve_batch(self._h, n, count, length, u.ctypes.data if n else None, out.ctypes.data if n else None))
        return out

    def _hash_to_curve(self, suite, msgs, dst):
        dst = _h2c_dst(dst)
        n, blob, offs = _h2c_messages(msgs)
        out = self._points_out(n)
        self._check(self._lib.s2k_hash_to_curve_batch(self._h, suite, n, dst, len(dst), blob.ctypes.data, offs.ctypes.data, 0,
                                                      out.ctypes.data if n else None))
        return out

    def hash_to_curve(self, msgs, dst) -> np.ndarray:
        """Secp256k1_XMD_SHA256_SSWU_RO(dst, msg) for every message (h2c.go:25-45): (n, 65) records."""
        return self._hash_to_curve(H2C_SSWU_RO, msgs, dst)

    def encode_to_curve(self, msgs, dst) -> np.ndarray:
        """Secp256k1_XMD_SHA256_SSWU_NU(dst, msg) for every message (h2c.go:49-63): (n, 65) records."""
        return self._hash_to_curve(H2C_SSWU_NU, msgs, dst)

    def hash_to_curve_device(self, suite, n, dst, d_msgs, d_msg_offsets, msg_len, total_msg_bytes, d_out, stream=0):
        """s2k_hash_to_curve_batch_device: device pointers (d_msg_offsets None: n messages of msg_len bytes), the tag on the
        host; d_out: n * 65 bytes.  Synchronises `stream` once."""
        dst = _h2c_dst(dst)
        self._check(self._lib.s2k_hash_to_curve_batch_device(self._h, int(suite), int(n), dst, len(dst), d_msgs, d_msg_offsets,
                                                             int(msg_len), int(total_msg_bytes), d_out, stream))

    def point_decode_batch(self, enc, enc_len):
        enc = _arr(enc, enc_len)
        n = enc.shape[0]
        out, ok = self._points_out(n), np.zeros(n, dtype=np.uint8)
        self._check(self._lib.s2k_point_decode_batch(self._h, n, enc_len, enc.ctypes.data, out.ctypes.data, ok.ctypes.data))
        return out, ok

    # ---- field / scalar -------------------------------------------------------------
    def _field(self, fn, op, a, b):
        a = _arr(a, 32)
        n = a.shape[0]
        bb = _arr(b, 32, n) if b is not None else None
        out, flag = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(fn(self._h, op, n, a.ctypes.data, bb.ctypes.data if bb is not None else None, out.ctypes.data,
                       flag.ctypes.data))
        return out, flag

    def fp_op_batch(self, op, a, b=None):
        return self._field(self._lib.s2k_fp_op_batch, op, a, b)

    def fn_op_batch(self, op, a, b=None):
        return self._field(self._lib.s2k_fn_op_batch, op, a, b)

    def fn_split_glv_batch(self, k):
        k = _arr(k, 32)
        n = k.shape[0]
        k1, k2 = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
        self._check(self._lib.s2k_fn_split_glv_batch(self._h, n, k.ctypes.data, k1.ctypes.data, k2.ctypes.data))
        return k1, k2

    def generator_window_bits(self) -> int:
        """window bits of the generator tables this context's launches use NOW (gt_info; the library's target width is
        s2k_generator_window_bits)"""
        return self.gt_info()["bits"]

    def gtable_entry(self, i, d) -> bytes:
        out = np.zeros(64, dtype=np.uint8)
        self._check(self._lib.s2k_debug_gtable_entry(self._h, i, d, out.ctypes.data))
        return out.tobytes()


class Ticket:
    """A batch in flight (s2k_ticket): wait() blocks until its verdicts are there and returns them.  The arrays of the batch
    belong to the owner (Engine / Group) until then: dropping a Ticket is safe."""

    def __init__(self, owner, ticket, out):
        self._owner, self.ticket, self._out = owner, ticket, out
        self._done = False

    def wait(self) -> np.ndarray:
        if not self._done:
            self._owner._wait(self.ticket)
            self._done = True
            self._owner._release(self.ticket)
        return self._out

    def done(self) -> bool:
        """s2k_poll: True once the verdicts are delivered (never blocks)."""
        if not self._done and hasattr(self._owner, "_poll") and self._owner._poll(self.ticket):
            self._done = True
            self._owner._release(self.ticket)
        return self._done


def device_count() -> int:
    """Devices the HIP runtime sees (s2k_device_count); 0 without a GPU."""
    return int(load_library().s2k_device_count())


class Group(_TicketOwner):
    """Several devices behind one process (s2k_group): one context and one host thread per listed device, contiguous
    index shards, verdicts written straight into the result array."""

    def __init__(self, devices, gt_bits: int = 0, wait_tables: bool = False):
        """gt_bits / wait_tables: as Engine's (s2k_group_create_ex): every member, and its child contexts, on that table width."""
        self._lib = load_library()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._lib.s2k_group_create_ex(devs, len(devices), int(gt_bits), CTX_WAIT_TABLES if wait_tables else 0, C.byref(h))
        if rc != 0:
            raise EngineError(f"s2k_group_create_ex failed ({rc})")
        self._h = h
        self.devices = list(devices)
        import weakref
        self._keysets = weakref.WeakSet()     # key sets go before their group (s2k_group_keyset_destroy follows the group pointer)

    def close(self):
        if getattr(self, "_h", None):
            for ks in list(self._keysets):
                ks.close()
            self._lib.s2k_group_destroy(self._h)    # (finishes the batches in flight first; frees the group's host blocks)
            self._h = None
            self._inflight = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._lib.s2k_group_size(self._h))

    def _check(self, rc):
        if rc != 0:
            raise EngineError(f"group call failed ({rc}): {self._lib.s2k_group_last_error(self._h).decode()}")

    def _wait(self, ticket):
        self._check(self._lib.s2k_group_wait(self._h, ticket))

    def set_key_grouping(self, mode: int = KEYS_AUTO, min_group: int = 0, hash_bits: int = 0, max_tables: int = 0):
        self._check(self._lib.s2k_group_set_key_grouping(self._h, int(mode), int(min_group), int(hash_bits), int(max_tables)))

    def set_small_batch_max(self, max_n: int):
        self._check(self._lib.s2k_group_set_small_batch_max(self._h, int(max_n)))

    def set_mid_batch_max(self, max_n: int):
        self._check(self._lib.s2k_group_set_mid_batch_max(self._h, int(max_n)))

    def set_keyset_small_batch_max(self, max_n: int):
        self._check(self._lib.s2k_group_set_keyset_small_batch_max(self._h, int(max_n)))

    def set_keyset_comb_small_batch_max(self, max_n: int):
        self._check(self._lib.s2k_group_set_keyset_comb_small_batch_max(self._h, int(max_n)))

    def gt_wait(self) -> int:
        """block until every member's device has its wide generator tables (s2k_group_gt_wait); the smallest width in use"""
        return int(self._lib.s2k_group_gt_wait(self._h))

    def shard_size(self, n: int) -> int:
        """items per member of a batch of n (s2k_group_shard_size)"""
        return int(self._lib.s2k_group_shard_size(self._h, int(n)))

    def host_alloc(self, n: int, width: int) -> np.ndarray:
        """An (n, width) uint8 array in page-locked memory whose shard ranges lie on the NUMA node of the member that will read
        them (s2k_group_host_alloc).  The memory belongs to the group: it is freed by host_free() or with the group, and the
        array must not be used after that."""
        p = self._lib.s2k_group_host_alloc(self._h, int(width), int(n))
        if not p:
            raise EngineError(f"s2k_group_host_alloc failed: {self._lib.s2k_group_last_error(self._h).decode()}")
        a = np.ctypeslib.as_array((C.c_uint8 * (n * width)).from_address(p)).reshape(n, width)
        return a

    def host_free(self, a: np.ndarray):
        self._lib.s2k_group_host_free(self._h, a.ctypes.data)

    def member_stats_ex(self):
        """Per member: dict(n, lo, ms, device, numa_node, bound_cpus, h2d_ms, device_ms) of its last finished shard
        (s2k_group_member_stats_ex; the device-clock times are zero until a shard has run after the first call)."""
        m = len(self)
        st = np.zeros(8 * m, dtype=np.float64)
        self._check(self._lib.s2k_group_member_stats_ex(self._h, st.ctypes.data))
        keys = ("n", "lo", "ms", "device", "numa_node", "bound_cpus", "h2d_ms", "device_ms")
        return [dict(zip(keys, st[8 * i:8 * i + 8].tolist())) for i in range(m)]

    def ecdsa_verify_batch_submit(self, pub_xy, digest32, r, s, out=None, reject_malleable: bool = False) -> Ticket:
        arrs = [(_arr(a, w) if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]) else a.reshape(-1, w))
                for a, w in ((pub_xy, 64), (digest32, 32), (r, 32), (s, 32))]
        n = arrs[2].shape[0]
        if any(a.shape[0] != n for a in arrs):
            raise ValueError("length mismatch")
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_group_ecdsa_verify_batch_submit(self._h, n, arrs[0].ctypes.data, arrs[1].ctypes.data,
                                                                  arrs[2].ctypes.data, arrs[3].ctypes.data,
                                                                  REJECT_MALLEABLE if reject_malleable else 0, out.ctypes.data,
                                                                  C.byref(t)))
        return self._hold(int(t.value), out, arrs)

    def ecdsa_verify_batch(self, pub_xy, digest32, r, s, reject_malleable: bool = False) -> np.ndarray:
        return self.ecdsa_verify_batch_submit(pub_xy, digest32, r, s, reject_malleable=reject_malleable).wait()

    def ecdsa_verify_encoded_batch_submit(self, pubs, digests, sigs, encoding=ENCODING_ASN1, digest_len=0,
                                          reject_malleable=False, bip0066=False) -> Ticket:
        """s2k_group_ecdsa_verify_encoded_batch_submit for lists of byte strings (or pre-built (blob, offsets) pairs)."""
        def cat(x):
            return x if isinstance(x, tuple) else _concat(list(x))
        (pb, po), (db, do), (sb, so) = cat(pubs), cat(digests), cat(sigs)
        n = len(po) - 1
        if len(do) - 1 != n or len(so) - 1 != n:
            raise ValueError("length mismatch")
        out = np.zeros(n, dtype=np.uint8)
        flags = (REJECT_MALLEABLE if reject_malleable else 0) | (BIP0066 if bip0066 else 0)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_group_ecdsa_verify_encoded_batch_submit(self._h, n, pb.ctypes.data, po.ctypes.data, db.ctypes.data,
                                                                          do.ctypes.data, sb.ctypes.data, so.ctypes.data, encoding,
                                                                          digest_len, flags, out.ctypes.data, C.byref(t)))
        return self._hold(int(t.value), out, [pb, po, db, do, sb, so])

    def schnorr_batch_verify_rlc(self, pk32, msgs, sig64, seed32: bytes | None = None) -> bool:
        """BIP-340 whole-batch check with the signatures sharded over the members (s2k_group_schnorr_batch_verify_rlc)."""
        pk32 = _arr(pk32, 32)
        n = pk32.shape[0]
        sig64 = _arr(sig64, 64, n)
        seed = np.frombuffer(seed32 if seed32 is not None else os.urandom(32), dtype=np.uint8)
        res = C.c_int(0)
        if isinstance(msgs, (list, tuple)):
            offs = np.zeros(n + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
            blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
            self._check(self._lib.s2k_group_schnorr_batch_verify_rlc(self._h, n, pk32.ctypes.data, blob.ctypes.data, offs.ctypes.data, 0,
                                                                     sig64.ctypes.data, seed.ctypes.data, C.byref(res)))
        else:
            m = np.ascontiguousarray(msgs, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 0), np.uint8)
            self._check(self._lib.s2k_group_schnorr_batch_verify_rlc(self._h, n, pk32.ctypes.data, m.ctypes.data if m.size else None, None,
                                                                     m.shape[1], sig64.ctypes.data, seed.ctypes.data, C.byref(res)))
        return bool(res.value)

    def multi_scalar_mult(self, scalars, points) -> bytes:
        """sum of scalars[i] * points[i] with the terms sharded over the members (s2k_group_multi_scalar_mult) -> 65-byte record"""
        k = _arr(scalars, 32)
        n = k.shape[0]
        p = _arr(points, 65, n)
        out = np.zeros(65, dtype=np.uint8)
        self._check(self._lib.s2k_group_multi_scalar_mult(self._h, n, k.ctypes.data, p.ctypes.data, out.ctypes.data))
        return out.tobytes()

    def keyset_create(self, pub_xy, layout: int = 0, capacity: int = 0) -> "GroupKeySet":
        """The tables of a list of public keys on every member's device (s2k_group_keyset_create_cap); capacity: keys every
        member's set has memory for (0: as many as pub_xy holds)."""
        return GroupKeySet(self, pub_xy, layout, capacity)

    def ecdsa_verify_batch_keyset_submit(self, keyset, key_index, digest32, r, s, out=None, reject_malleable: bool = False) -> Ticket:
        ki = np.ascontiguousarray(key_index, dtype=np.uint32).reshape(-1)
        n = ki.shape[0]
        arrs = [ki] + [(_arr(a, 32) if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]) else a.reshape(-1, 32))
                       for a in (digest32, r, s)]
        if any(a.shape[0] != n for a in arrs):
            raise ValueError("length mismatch")
        out = _out_array(out, n)
        t = C.c_uint64(0)
        self._check(self._lib.s2k_group_ecdsa_verify_batch_keyset_submit(self._h, keyset._k, n, arrs[0].ctypes.data, arrs[1].ctypes.data,
                                                                         arrs[2].ctypes.data, arrs[3].ctypes.data,
                                                                         REJECT_MALLEABLE if reject_malleable else 0, out.ctypes.data,
                                                                         C.byref(t)))
        return self._hold(int(t.value), out, arrs + [keyset])

    def ecdsa_verify_batch_keyset(self, keyset, key_index, digest32, r, s, reject_malleable: bool = False) -> np.ndarray:
        return self.ecdsa_verify_batch_keyset_submit(keyset, key_index, digest32, r, s, reject_malleable=reject_malleable).wait()

    def member_stats(self):
        """Per member, of its last finished shard: dict(n, first, ms, device)."""
        st = (C.c_double * (4 * len(self)))()
        self._check(self._lib.s2k_group_member_stats(self._h, st))
        return [{"n": int(st[4 * i]), "first": int(st[4 * i + 1]), "ms": float(st[4 * i + 2]), "device": int(st[4 * i + 3])}
                for i in range(len(self))]


class GroupKeySet:
    """Handle of s2k_group_keyset_*: the per-key tables of a key list on every device of a group."""

    def __init__(self, group: "Group", pub_xy, layout: int = 0, capacity: int = 0):
        pub_xy = _arr(pub_xy, 64)
        self._grp = group
        k = C.c_void_p()
        group._check(group._lib.s2k_group_keyset_create_cap(group._h, pub_xy.shape[0], pub_xy.ctypes.data, int(layout), int(capacity),
                                                            C.byref(k)))
        self._k = k
        group._keysets.add(self)

    def capacity(self) -> int:
        """keys every member's set has memory for (s2k_group_keyset_capacity)"""
        return int(self._grp._lib.s2k_group_keyset_capacity(self._k))

    def reserve(self, capacity: int):
        """s2k_group_keyset_reserve: memory for `capacity` keys on every member"""
        self._grp._check(self._grp._lib.s2k_group_keyset_reserve(self._k, int(capacity)))

    def append(self, pub_xy) -> int:
        """s2k_group_keyset_append: more keys (n x 64 bytes) on every member's set; the index of the first of them"""
        pub_xy = _arr(pub_xy, 64)
        first = C.c_uint32(0)
        self._grp._check(self._grp._lib.s2k_group_keyset_append(self._k, pub_xy.shape[0], pub_xy.ctypes.data if pub_xy.shape[0] else None,
                                                                C.byref(first)))
        return int(first.value)

    def replace(self, slots, pub_xy):
        """s2k_group_keyset_replace: the live rows `slots` of every member's set overwritten with the keys pub_xy (host)"""
        slots, pub_xy = _slots(slots), _arr(pub_xy, 64)
        m = slots.shape[0]
        if pub_xy.nbytes != m * 64:
            raise ValueError("secp256k1: len(slots) * 64 != len(pub_xy)")
        self._grp._check(self._grp._lib.s2k_group_keyset_replace(self._k, m, slots.ctypes.data if m else None, pub_xy.ctypes.data if m else None))

    def remove(self, slots):
        """s2k_group_keyset_remove: the live rows `slots` of every member's set made "no key" """
        slots = _slots(slots)
        m = slots.shape[0]
        self._grp._check(self._grp._lib.s2k_group_keyset_remove(self._k, m, slots.ctypes.data if m else None))

    def layout(self) -> int:
        return int(self._grp._lib.s2k_group_keyset_layout(self._k))

    def __len__(self):
        return int(self._grp._lib.s2k_group_keyset_size(self._k))

    def device_bytes(self):
        """per member"""
        return int(self._grp._lib.s2k_group_keyset_device_bytes(self._k))

    def close(self):
        if self._k and self._grp._h:
            self._grp._lib.s2k_group_keyset_destroy(self._k)
        self._k = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PointSet:
    """Handle of s2k_pointset_*: the multiples mag * 2^(c pos) * P of a fixed list of points on the engine's device."""

    def __init__(self, engine: "Engine", points, window_bits: int = 0):
        points = _arr(points, 65)
        self._eng = engine
        k = C.c_void_p()
        engine._check(engine._lib.s2k_pointset_create(engine._h, points.shape[0], points.ctypes.data, int(window_bits), C.byref(k)))
        self._k = k

    def __len__(self):
        return int(self._eng._lib.s2k_pointset_size(self._k))

    def window_bits(self) -> int:
        return int(self._eng._lib.s2k_pointset_window_bits(self._k))

    def device_bytes(self) -> int:
        return int(self._eng._lib.s2k_pointset_device_bytes(self._k))

    def entry(self, i: int, pos: int, mag: int) -> bytes:
        """Table entry (pos, mag) of point i as X || Y (s2k_debug_pointset_entry); 64 zero bytes for an identity record."""
        out = np.zeros(64, dtype=np.uint8)
        self._eng._check(self._eng._lib.s2k_debug_pointset_entry(self._k, int(i), int(pos), int(mag), out.ctypes.data))
        return out.tobytes()

    def multi_scalar_mult_segments(self, scalars, offsets, point_index=None) -> np.ndarray:
        """out[j] = sum of scalars[i] * P[point_index[i]] over offsets[j] <= i < offsets[j + 1], P the points of the set:
        (n_seg, 65) records, those of Engine.multi_scalar_mult_segments on the expanded point array.  point_index None: the
        term at position t of its segment uses point t.  Public scalars only."""
        scalars = _arr(scalars, 32)
        n = scalars.shape[0]
        off = check_segment_offsets(offsets, n)
        n_seg = off.shape[0] - 1
        idx = None
        if point_index is not None:
            idx = np.ascontiguousarray(np.asarray(point_index, dtype=np.uint32).reshape(-1))
            if idx.shape[0] != n:
                raise ValueError("secp256k1: len(scalars) != len(point_index)")
        out = np.zeros((n_seg, 65), dtype=np.uint8)
        e = self._eng
        e._check(e._lib.s2k_pointset_multi_scalar_mult_segments(e._h, self._k, n, scalars.ctypes.data if n else None,
                                                                idx.ctypes.data if idx is not None else None, n_seg, off.ctypes.data,
                                                                out.ctypes.data if n_seg else None))
        return out

    def multi_scalar_mult_segments_device(self, n, d_scalars, d_point_index, offsets, d_out, stream=0):
        """The same on device buffers (d_point_index: n uint32 or None; d_out: n_seg * 65 bytes); `offsets` stays host memory.
        Synchronises `stream` once."""
        off = check_segment_offsets(offsets, int(n))
        e = self._eng
        e._check(e._lib.s2k_pointset_multi_scalar_mult_segments_device(e._h, self._k, int(n), d_scalars, d_point_index, off.shape[0] - 1,
                                                                       off.ctypes.data, d_out, stream))

    def close(self):
        if self._k:
            self._eng._lib.s2k_pointset_destroy(self._k)
            self._k = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeySet:
    """Handle of s2k_keyset_*: the per-key tables of a key list on the engine's device.  len(): the keys it holds."""

    def __init__(self, engine: "Engine", pub_xy, layout: int = 0, capacity: int = 0):
        pub_xy = _arr(pub_xy, 64)
        self._eng = engine
        k = C.c_void_p()
        engine._check(engine._lib.s2k_keyset_create_cap(engine._h, pub_xy.shape[0], pub_xy.ctypes.data, int(layout), int(capacity),
                                                        C.byref(k)))
        self._k = k

    def _check_own(self, rc):
        # (these calls take no context: their message is the calling thread's)
        if rc != 0:
            raise EngineError(f"s2k error {rc}: {self._eng._lib.s2k_last_error(None).decode()}")

    def capacity(self) -> int:
        """keys the set has memory for (s2k_keyset_capacity); len() of them have tables"""
        return int(self._eng._lib.s2k_keyset_capacity(self._k))

    def reserve(self, capacity: int):
        """Memory for `capacity` keys (s2k_keyset_reserve): new buffers, the set copied over on the device.  Needs room for
        both copies for a moment: give a large set its capacity at creation.  A smaller capacity changes nothing."""
        self._check_own(self._eng._lib.s2k_keyset_reserve(self._k, int(capacity)))

    def append(self, pub_xy) -> int:
        """More keys (n x 64 bytes: host bytes / arrays, or a torch uint8 tensor on the set's device), within the capacity
        (s2k_keyset_append[_device]): only their tables are built, and the set's index follows.  Returns the index of the
        first of them.  No call or ticket that uses the set may be in progress."""
        first = C.c_uint32(0)
        if hasattr(pub_xy, "data_ptr") and hasattr(pub_xy, "is_cuda"):
            t = pub_xy
            if not t.is_cuda or t.element_size() != 1 or t.numel() % 64:
                raise ValueError("secp256k1: a device tensor of n x 64 bytes")
            t = t.contiguous()
            n = t.numel() // 64
            self._check_own(self._eng._lib.s2k_keyset_append_device(self._k, n, t.data_ptr() if n else None, C.byref(first)))
            return int(first.value)
        pub_xy = _arr(pub_xy, 64)
        n = pub_xy.shape[0]
        self._check_own(self._eng._lib.s2k_keyset_append(self._k, n, pub_xy.ctypes.data if n else None, C.byref(first)))
        return int(first.value)

    def replace(self, slots, pub_xy):
        """The live rows `slots` (uint32, each below len(), none twice) overwritten with the keys pub_xy (len(slots) x 64 bytes:
        host bytes / arrays, or a torch uint8 tensor on the set's device) - s2k_keyset_replace[_device].  Afterwards the set is,
        in every call, the set created whole from the changed key list; len(), capacity() and every other row's index stay, and
        the set's index follows.  Which rows are free to reuse is the caller's bookkeeping.  No call or ticket that uses the set
        may be in progress."""
        slots = _slots(slots)
        m = slots.shape[0]
        if hasattr(pub_xy, "data_ptr") and hasattr(pub_xy, "is_cuda"):
            t = pub_xy
            if not t.is_cuda or t.element_size() != 1 or t.numel() != m * 64:
                raise ValueError("secp256k1: a device tensor of len(slots) x 64 bytes")
            t = t.contiguous()
            self._check_own(self._eng._lib.s2k_keyset_replace_device(self._k, m, slots.ctypes.data if m else None, t.data_ptr() if m else None))
            return
        pub_xy = _arr(pub_xy, 64)
        if pub_xy.nbytes != m * 64:
            raise ValueError("secp256k1: len(slots) * 64 != len(pub_xy)")
        self._check_own(self._eng._lib.s2k_keyset_replace(self._k, m, slots.ctypes.data if m else None, pub_xy.ctypes.data if m else None))

    def remove(self, slots):
        """The live rows `slots` made "no key" (s2k_keyset_remove: replace with 64 zero bytes each): every signature under them
        verifies false, valid_keys() says 0 and the lookups of valid keys never answer them.  The rows stay rows: len() does not
        move, and replace() puts a key back."""
        slots = _slots(slots)
        m = slots.shape[0]
        self._check_own(self._eng._lib.s2k_keyset_remove(self._k, m, slots.ctypes.data if m else None))

    def layout(self) -> int:
        """The layout the set has: KEYSET_CHUNKS, KEYSET_JOINT, KEYSET_JOINT5, KEYSET_JOINT6 or KEYSET_COMB (s2k_keyset_layout)."""
        return int(self._eng._lib.s2k_keyset_layout(self._k))

    def __len__(self):
        return int(self._eng._lib.s2k_keyset_size(self._k))

    def device_bytes(self):
        return int(self._eng._lib.s2k_keyset_device_bytes(self._k))

    def valid_keys(self) -> np.ndarray:
        out = np.zeros(len(self), dtype=np.uint8)
        self._eng._check(self._eng._lib.s2k_keyset_valid_keys(self._k, out.ctypes.data))
        return out

    def debug_entries(self, key: int, section: int, first: int = 0, count: int | None = None) -> np.ndarray:
        """test hook (s2k_debug_keyset_entries): entries first .. first + count - 1 (None: to the end of the section) of the
        tables of key `key`, read with the ladders' loaders.  Section 0: the key's shared scale W, a (1, 32) array; section 1:
        the base table, (count, 96) = X || Y || beta X; section 2: the joint table, (count, 64) = X || Y.  Coordinates are 32
        big-endian bytes, reduced - but for the wide joint layouts, whose stored words come as they are.  The sections' sizes
        (s2k_debug_keyset_section_entries) and what each entry is: include/secp256k1_voi_amd.h.  Whatever the library refuses -
        a section the layout lacks, a range past its end - raises EngineError."""
        if count is None:
            total = C.c_size_t(0)
            self._check_own(self._eng._lib.s2k_debug_keyset_section_entries(self._k, int(section), C.byref(total)))
            count = max(int(total.value) - int(first), 0)     # (a `first` past the end: the library refuses it below)
        out = np.zeros((int(count), {0: 32, 1: 96}.get(int(section), 64)), dtype=np.uint8)
        self._check_own(self._eng._lib.s2k_debug_keyset_entries(self._k, int(key), int(section), int(first), int(count), out.ctypes.data))
        return out

    def index_create(self, log2_slots: int = 0):
        """Build the set's index, key bytes -> key index, once (s2k_keyset_index_create): 2^log2_slots slots of 8 bytes, more
        than the set has keys; 0: keyset_index_geometry's choice.  Engine.keyset_lookup and ecdsa_verify_batch_bykey need it."""
        rc = self._eng._lib.s2k_keyset_index_create(self._k, int(log2_slots))
        if rc != 0:
            raise EngineError(f"s2k error {rc}: {self._eng._lib.s2k_last_error(None).decode()}")

    def index_info(self) -> dict:
        """slots (0: no index), bytes, occupied slots (= distinct 64-byte keys), longest probe distance (s2k_keyset_index_info)"""
        out = np.zeros(4, dtype=np.uint64)
        self._eng._check(self._eng._lib.s2k_keyset_index_info(self._k, out.ctypes.data))
        return dict(slots=int(out[0]), bytes=int(out[1]), occupied=int(out[2]), longest_probe=int(out[3]))

    def close(self):
        if self._k:
            self._eng._lib.s2k_keyset_destroy(self._k)
            self._k = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
