"""ctypes binding of libeigenface.so (include/eigenface.h).

The product path has no CPU fallback: if the HIP library is missing or cannot be
loaded, every entry point raises ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lib", "libeigenface.so")
# diagnostic builds (instrumented / ablated kernels, never a non-HIP fallback) by name
if os.environ.get("EF_LIB_VARIANT"):
    LIB_PATH = LIB_PATH.replace("libeigenface.so", f"libeigenface_{os.environ['EF_LIB_VARIANT']}.so")

EF_OK = 0
EF_U8, EF_F32, EF_F64 = 0, 1, 2
EF_METRIC_L2, EF_METRIC_COSINE = 0, 1
EF_FIT_STANDARDIZE = 0x1
EF_MODEL_BF16 = 0x2
EF_MEM_DEVICE = 0x100
EF_IMG_RGB = 0x200
EF_ROI_RECTS_DEVICE = 0x400
EF_BANK_GATE_RELATIVE = 0x800
EF_KERNEL_SEARCH, EF_KERNEL_PROJECT, EF_KERNEL_TMATCH, EF_KERNEL_INGEST, EF_KERNEL_HAAR, EF_KERNEL_JPEG, \
    EF_KERNEL_SYRK, EF_KERNEL_JPEG_HOST = 0, 1, 2, 3, 4, 5, 6, 7
EF_KERNEL_SCAN = 8
EF_KERNEL_RECON, EF_KERNEL_RECON_REDUCE = 9, 10
EF_KERNEL_HAAR_SCAN = 11
EF_KERNEL_CLUSTER = 12
EF_KERNEL_RANGE = 13
EF_KERNEL_RANK = 14
EF_RANK_GENUINE_GIVEN = 0x1000  # ef_search_rank: genuine[b] is an input
EF_CLUSTER_UNCONVERGED = 1 << 62  # ef_gallery_cluster: bit of info[3] on a device call
EF_HAAR_GROUP_MAX = 16384  # rectangles per grouping; the ceiling of a Haar scan plan's max_candidates
EF_HAAR_SCAN_OVERFLOW, EF_HAAR_SCAN_UNCONVERGED = 0x1, 0x2  # ef_haar_scan_head.status bits
EF_JPEG_GRAY, EF_JPEG_BGR = 0, 1
EF_JPEG_E_UNSUPPORTED, EF_JPEG_E_CORRUPT = -10, -11
EF_KEY_NONE = (1 << 63) - 1
EF_UNIQUE_ID_BYTES = 128
EF_OPT_FIT_MAX_ITERS, EF_OPT_FIT_FP32_COARSE, EF_OPT_COV_SLAB_BYTES, EF_OPT_TM_INT64_SUMS, EF_OPT_HAAR_ORDERED = \
    1, 2, 3, 4, 5
EF_OPT_JPEG_CHUNK_BITS = 6
EF_OPT_SEARCH_SPLIT_BF16 = 7
EF_OPT_JPEG_PART_FILES = 8
EF_OPT_FIT_CHEBYSHEV = 9
EF_OPT_HOST_THREADS = 10
EF_OPT_SEARCH_PREFIX = 11
EF_OPT_SEARCH_TOPK_CAND = 12
EF_OPT_SEARCH_PREFIX_SPLIT = 13
EF_OPT_PROJECT_SPLIT_BF16 = 14
EF_OPT_RANK_BITMAP_BYTES = 15
EF_OPT_SEARCH_PREFIX_SCREEN = 16
EF_TOPK_MAX = 64  # most ranks of a top-m search
EF_LABEL_SAME, EF_LABEL_OTHER, EF_LABEL_ANY = 0, 1, 2  # ef_search_labelled relations
EF_CENSUS_MAX_BINS = 2048  # most bins of ef_score_census
EF_BANK_MAX_MODELS = 4096
EF_BANK_MAX_PROBES = 4096  # per ef_bank_recognize call
EF_E_INVALID, EF_E_STATE = -1, -3
EF_E_NUMERIC = -5


class ef_scan_det(C.Structure):
    """include/eigenface.h ef_scan_det: one group's detection of a scanned frame."""
    _fields_ = [("found", C.c_int32), ("problem", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32),
                ("h", C.c_int32), ("confidence", C.c_float), ("pad", C.c_int32)]


# numpy view of an ef_haar_scan_head
HAAR_SCAN_HEAD_DTYPE = [("status", "<i4"), ("n_candidates", "<i4"), ("n_rects", "<i4"), ("n_faces", "<i4")]

# numpy view of an ef_scan_det array
SCAN_DET_DTYPE = [("found", "<i4"), ("problem", "<i4"), ("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"),
                  ("confidence", "<f4"), ("pad", "<i4")]


class ef_match(C.Structure):
    """include/eigenface.h ef_match: fp64 winner score, tie-tolerance scale, packed key."""
    _fields_ = [("score", C.c_double), ("scale", C.c_double), ("key", C.c_int64)]


# numpy view of an ef_match array
MATCH_DTYPE = [("score", "<f8"), ("scale", "<f8"), ("key", "<i8")]

_ERRNAMES = {-1: "EF_E_INVALID", -2: "EF_E_HIP", -3: "EF_E_STATE", -4: "EF_E_NOMEM", -5: "EF_E_NUMERIC"}


class NativeLibraryError(RuntimeError):
    """libeigenface.so is missing or unusable (there is no CPU fallback)."""


class EigenfaceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


_lock = threading.Lock()
_lib = None

vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32

_SIGS = {
    "ef_api_version": ([], C.c_int),
    "ef_device_count": ([C.POINTER(C.c_int)], C.c_int),
    "ef_create": ([C.c_int, C.POINTER(vp)], C.c_int),
    "ef_destroy": ([vp], None),
    "ef_last_error": ([vp], C.c_char_p),
    "ef_set_stream": ([vp, vp], C.c_int),
    "ef_use_own_stream": ([vp], C.c_int),
    "ef_get_stream": ([vp, C.POINTER(vp)], C.c_int),
    "ef_synchronize": ([vp], C.c_int),
    "ef_trim": ([vp], C.c_int),
    "ef_fit": ([vp, vp, i64, i64, i32, u32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)], C.c_int),
    "ef_fit_ex": ([vp, vp, i32, i64, i64, i32, u32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)],
                  C.c_int),
    "ef_colstats": ([vp, vp, i32, i64, i64, u32, vp, vp], C.c_int),
    "ef_chol_inv": ([vp, vp, i32, i64, C.c_double, vp, vp], C.c_int),
    "ef_fit_shard_stats": ([vp, vp, i64, i64, vp, vp, vp, u32], C.c_int),
    "ef_fit_from_stats": ([vp, vp, vp, vp, i64, i64, i32, u32, vp, vp, vp, vp, vp, vp, C.POINTER(i32),
                           C.POINTER(i32)], C.c_int),
    "ef_fit_transform": ([vp, vp, i64, i64, vp, vp, vp, i32, u32, vp], C.c_int),
    "ef_model_set": ([vp, vp, vp, i64, i32, u32], C.c_int),
    "ef_project": ([vp, vp, i32, i64, vp, u32], C.c_int),
    "ef_gallery_set": ([vp, vp, i64, i32, i64, u32], C.c_int),
    "ef_search": ([vp, vp, i64, i32, vp, u32], C.c_int),
    "ef_recognize": ([vp, vp, i32, i64, i32, vp, vp, u32], C.c_int),
    "ef_keys_decode": ([vp, i64, i32, vp, vp], None),
    "ef_search_schedule": ([i64, i32, i64, i32, vp, i32, C.POINTER(i32)], C.c_int),
    "ef_search_matches": ([vp, vp, i64, i32, vp, u32], C.c_int),
    "ef_recognize_matches": ([vp, vp, i32, i64, i32, vp, vp, u32], C.c_int),
    "ef_matches_merge": ([vp, vp, i32, i64, vp, vp, u32], C.c_int),
    "ef_comm_unique_id": ([vp], C.c_int),
    "ef_comm_init": ([vp, i32, i32, vp], C.c_int),
    "ef_comm_destroy": ([vp], C.c_int),
    "ef_comm_info": ([vp, C.POINTER(i32), C.POINTER(i32)], C.c_int),
    "ef_set_option": ([vp, i32, i64], C.c_int),
    "ef_get_option": ([vp, i32, C.POINTER(i64)], C.c_int),
    "ef_preprocess": ([vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, u32], C.c_int),
    "ef_jpeg_info": ([vp, vp, vp, i32, vp, vp, vp, vp], C.c_int),
    "ef_jpeg_decode": ([vp, vp, vp, vp, i32, i32, vp, vp, vp, u32], C.c_int),
    "ef_jpeg_ingest": ([vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, u32], C.c_int),
    "ef_tm_prepare": ([vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32, u32], C.c_int),
    "ef_tm_match": ([vp, vp, i64, vp, vp, vp, vp, u32], C.c_int),
    "ef_tm_info": ([vp, C.POINTER(i32), C.POINTER(i64), vp, vp], C.c_int),
    "ef_tm_sums_bits": ([i32, i32, i64], C.c_int),
    "ef_haar_set_cascade": ([vp, i32, i32, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp], C.c_int),
    "ef_haar_detect": ([vp, vp, i32, i32, i64, C.c_double, i32, i32, i32, i32, i32, vp, i32, C.POINTER(i32), vp, i32,
                        C.POINTER(i32), u32], C.c_int),
    "ef_timing_enable": ([vp, C.c_int], C.c_int),
    "ef_timing_get": ([vp, i32, C.POINTER(C.c_double), C.POINTER(i64)], C.c_int),
    "ef_timing_reset": ([vp], C.c_int),
    "ef_search_stats": ([vp, C.POINTER(i64)], C.c_int),
    "ef_prefix_screen_stats": ([vp, C.POINTER(i64)], C.c_int),  # added by symbol
    "ef_search_topk": ([vp, vp, i64, i32, i32, vp, u32], C.c_int),
    "ef_recognize_topk": ([vp, vp, i32, i64, i32, i32, vp, vp, u32], C.c_int),
    "ef_search_topk_matches": ([vp, vp, i64, i32, i32, vp, u32], C.c_int),
    "ef_matches_merge_topk": ([vp, vp, i32, i64, i32, vp, vp, u32], C.c_int),
    "ef_search_topk_stats": ([vp, C.POINTER(i64)], C.c_int),
    # labelled search: added by symbol, EF_API_VERSION stays 7
    "ef_gallery_labels": ([vp, vp, i64, u32], C.c_int),
    "ef_search_labelled": ([vp, vp, i64, i32, i32, vp, vp, vp, vp, u32], C.c_int),
    # score census: added the same way
    "ef_score_census": ([vp, vp, i64, i32, vp, vp, C.c_float, C.c_float, i32, vp, u32], C.c_int),
    # gallery clustering: added the same way
    "ef_gallery_cluster": ([vp, i32, C.c_double, i32, vp, vp, vp, u32], C.c_int),
    "ef_cluster_schedule": ([i64, i32, vp, i32, C.POINTER(i32)], C.c_int),
    # range search: added the same way
    "ef_search_range": ([vp, vp, i64, i32, C.c_double, vp, vp, vp, vp, i64, vp, u32], C.c_int),
    "ef_search_range_plan": ([i64, i64, i32, C.POINTER(i64), C.POINTER(i64)], C.c_int),
    # identification rank: added the same way
    "ef_search_rank": ([vp, vp, i64, i32, vp, vp, vp, vp, vp, u32], C.c_int),
    "ef_search_rank_plan": ([i64, i64, i64, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)], C.c_int),
    # model bank: added after API v7 without a version bump, so bound (and checked) by symbol
    "ef_bank_clear": ([vp], C.c_int),
    "ef_bank_add": ([vp, vp, vp, i64, i32, vp, i64, u32, C.POINTER(i32)], C.c_int),
    "ef_bank_info": ([vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)], C.c_int),
    "ef_bank_recognize": ([vp, vp, i32, i64, i32, vp, vp, vp, vp, u32], C.c_int),
    "ef_bank_schedule": ([i64, i64, vp, i32, C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)],
                         C.c_int),
    # ROI ingest and frame scan: added the same way, bound by symbol
    "ef_preprocess_rois": ([vp, vp, i64, i32, i32, i32, vp, i64, i32, i32, vp, u32], C.c_int),
    "ef_scan_prepare": ([vp, vp, i32, i32, i32, C.c_double], C.c_int),
    "ef_scan_frame": ([vp, vp, i64, i32, i32, vp, vp, vp, vp, u32], C.c_int),
    # reconstruction and distance from face space: added the same way, bound by symbol
    "ef_recon_set": ([vp, vp, vp, i64, i32, u32], C.c_int),
    "ef_reconstruct": ([vp, vp, i64, i32, vp, u32], C.c_int),
    "ef_face_distance": ([vp, vp, i32, i64, vp, vp, vp, u32], C.c_int),
    # model bank: distance from face space per slot and the face gate, bound by symbol too
    "ef_bank_recon_set": ([vp, i32, vp, vp, u32], C.c_int),
    "ef_bank_face_distance": ([vp, vp, i32, i64, vp, vp, vp, u32], C.c_int),
    "ef_bank_recognize_gated": ([vp, vp, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, u32], C.c_int),
    "ef_scan_frame_gated": ([vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, u32], C.c_int),
    "ef_bank_recon_schedule": ([i64, i64, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)],
                               C.c_int),
    # Haar route in one call: rectangle grouping on the GPU and the fused frame, bound by symbol
    "ef_haar_group": ([vp, vp, i32, i32, vp, i32, vp, u32], C.c_int),
    "ef_haar_scan_prepare": ([vp, i32, i32, C.c_double, i32, i32, i32, i32, i32, i32, i32, i32, i32], C.c_int),
    "ef_haar_scan_info": ([vp, C.POINTER(i32), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)], C.c_int),
    "ef_haar_scan_frame": ([vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, u32], C.c_int),
    # Fisher discriminant: class scatter and the generalised eigenproblem, bound by symbol
    "ef_lda_order": ([vp, i64, i32, vp, vp], C.c_int),
    "ef_lda_scatter": ([vp, vp, i32, i64, i32, vp, i32, vp, vp, vp, vp, vp, u32], C.c_int),
    "ef_lda_fit": ([vp, vp, i32, i64, i32, vp, i32, i32, C.c_double, vp, vp, vp, vp, u32], C.c_int),
}

EXPORTED_SYMBOLS = tuple(_SIGS)


def _load_torch_runtime_first():
    """One HIP runtime per process.  torch's wheel bundles its own ``libamdhip64.so``
    (soname ``libamdhip64.so.7``) and its libraries NEED it by the file name
    ``libamdhip64.so``; libeigenface NEEDs the soname.  Loaded after torch, libeigenface
    binds to torch's already-mapped runtime; loaded first, it maps /opt/rocm's and a later
    ``import torch`` maps a second runtime, and whichever initialises second sees no GPU
    (``ef_create`` fails with EF_E_HIP, or torch reports no device).  So torch, when it is
    installed, is imported before the library is opened."""
    import importlib.util
    import sys
    if "torch" in sys.modules or importlib.util.find_spec("torch") is None:
        return
    import torch  # noqa: F401


def lib():
    """Load (once) and return the ctypes handle; raise loudly when unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `make -C face-detection-recognization-pca_amd` "
                "or __graft_entry__.build() (there is no CPU fallback)")
        _load_torch_runtime_first()
        try:
            h = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the box
            raise NativeLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (args, res) in _SIGS.items():
            fn = getattr(h, name)
            fn.argtypes = args
            fn.restype = res
        if h.ef_api_version() != 7:
            raise NativeLibraryError("libeigenface.so API version mismatch")
        _lib = h
        return h


def check(ctx, rc):
    if rc != EF_OK:
        msg = lib().ef_last_error(ctx)
        raise EigenfaceError(rc, msg.decode() if msg else "")
    return rc
