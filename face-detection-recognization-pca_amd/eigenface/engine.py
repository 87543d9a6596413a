"""Thin Python layer over the C ABI: one ``Engine`` per GPU.

Arrays may be NumPy (host; the call copies in/out and synchronises) or torch-ROCm
CUDA tensors (device; zero-copy, stream-ordered, no synchronisation).  One call must
not mix the two.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _native as N

METRICS = {"l2": N.EF_METRIC_L2, "cosine": N.EF_METRIC_COSINE}
_RELATIONS = {"same": N.EF_LABEL_SAME, "other": N.EF_LABEL_OTHER, "any": N.EF_LABEL_ANY}


def _is_dev(x):
    return x is not None and hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _host(x, dtype):
    a = np.ascontiguousarray(x, dtype=dtype)
    return a, a.ctypes.data


def _dev(x, torch_dtype):
    if x.dtype != torch_dtype:
        raise TypeError(f"expected {torch_dtype}, got {x.dtype}")
    if not x.is_contiguous():
        x = x.contiguous()
    return x, x.data_ptr()


def _ptr(a):
    return None if a is None else a.data_ptr() if _is_dev(a) else a.ctypes.data


def _empty(shape, dtype, device):
    """An uninitialised output: a NumPy array for ``device`` None, else a tensor on ``device``."""
    if device is None:
        return np.empty(shape, dtype)
    import torch
    return torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=device)


def _per_probe(x, np_dtype, name, q, dev):
    """(array or tensor, pointer) of one value per probe of q, or (None, None): a host array for
    host probes; for device probes a tensor on their device (an array is uploaded)."""
    if x is None:
        return None, None
    if dev:
        import torch
        if not _is_dev(x):
            x = torch.as_tensor(np.ascontiguousarray(x, dtype=np_dtype), device=q.device)
        x, xp = _dev(x, getattr(torch, np.dtype(np_dtype).name))
    else:
        x, xp = _host(x, np_dtype)
    if tuple(x.shape) != (q.shape[0],):
        raise ValueError(f"{name} must be ({q.shape[0]},), got {tuple(x.shape)}")
    return x, xp


def _gate_arg(gate, device, M):
    """(array or tensor, pointer) of a face gate (M,) float32: NumPy for ``device`` None, else a
    tensor on ``device`` (an array is uploaded)."""
    if device is None:
        g, gp = _host(gate, np.float32)
    else:
        import torch
        g = gate if _is_dev(gate) else torch.as_tensor(np.asarray(gate, np.float32), device=device)
        g, gp = _dev(g, torch.float32)
    if tuple(g.shape) != (M,):
        raise ValueError(f"gate must be ({M},), got {tuple(g.shape)}")
    return g, gp


def _frame_outputs(n, M, d, gated, device):
    """What every frame scan returns behind its route's own outputs: [keys (n, M) int64, best_slot
    (n,) int32, rows (n, d) uint8] and, gated, [dffs2, energy] (n, M) float32."""
    out = [_empty((n, M), np.int64, device), _empty(n, np.int32, device), _empty((n, d), np.uint8, device)]
    if gated:
        out += [_empty((n, M), np.float32, device), _empty((n, M), np.float32, device)]
    return out


_OPTIONS = {"fit_max_iters": N.EF_OPT_FIT_MAX_ITERS, "fit_fp32_coarse": N.EF_OPT_FIT_FP32_COARSE,
            "cov_slab_bytes": N.EF_OPT_COV_SLAB_BYTES, "tm_int64_sums": N.EF_OPT_TM_INT64_SUMS,
            "haar_ordered": N.EF_OPT_HAAR_ORDERED, "jpeg_chunk_bits": N.EF_OPT_JPEG_CHUNK_BITS,
            "search_split_bf16": N.EF_OPT_SEARCH_SPLIT_BF16, "jpeg_part_files": N.EF_OPT_JPEG_PART_FILES,
            "fit_chebyshev": N.EF_OPT_FIT_CHEBYSHEV, "host_threads": N.EF_OPT_HOST_THREADS,
            "search_prefix": N.EF_OPT_SEARCH_PREFIX, "search_topk_cand": N.EF_OPT_SEARCH_TOPK_CAND,
            "search_prefix_split": N.EF_OPT_SEARCH_PREFIX_SPLIT,
            "search_prefix_screen": N.EF_OPT_SEARCH_PREFIX_SCREEN,
            "project_split_bf16": N.EF_OPT_PROJECT_SPLIT_BF16, "rank_bitmap_bytes": N.EF_OPT_RANK_BITMAP_BYTES}


def host_cpu_share():
    """The job's CPU share for the library's host workers: OMP_NUM_THREADS when set (the
    GPU pool presets it to the job's share), else the affinity mask, capped at 16."""
    share = None
    v = os.environ.get("OMP_NUM_THREADS", "")
    if v.strip().isdigit() and int(v) > 0:
        share = int(v)
    if share is None:
        try:
            share = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            share = os.cpu_count() or 1
    return max(1, min(16, share))


def _option(o):
    return _OPTIONS[o] if isinstance(o, str) else int(o)


def _metric(m):
    if isinstance(m, str):
        return METRICS[m.lower()]
    return int(m)


@dataclass
class FitResult:
    """Outputs of the GPU fit (float64).  ``components`` is k x d (rows =
    eigenfaces, sklearn ``components_``); manual_pca's ``eigenfaces`` is its
    transpose."""

    mean: np.ndarray
    var: np.ndarray
    scale: np.ndarray
    components: np.ndarray
    eigenvalues: np.ndarray
    projection: np.ndarray | None
    total_var: float
    k: int
    iters: int


@dataclass
class LdaResult:
    """Outputs of the Fisher discriminant fit (float64; NumPy, or tensors for device input).
    ``scalings`` (k, m) maps features to the discriminant space: (f - anything) @ scalings
    differs between two rows by the within-class Mahalanobis distance."""

    scalings: np.ndarray
    eigenvalues: np.ndarray
    mean: np.ndarray
    class_means: np.ndarray
    classes: np.ndarray


_TORCH_READY = False


def _init_torch_first():
    """torch's HIP runtime must come up before this process's first libeigenface context,
    or torch reports no GPU afterwards (seen on the MI355X boxes) — so when torch is
    installed it is initialised here, whether or not the caller imported it yet."""
    global _TORCH_READY
    if _TORCH_READY:
        return
    _TORCH_READY = True
    torch = sys.modules.get("torch")
    if torch is None:
        import importlib.util
        if importlib.util.find_spec("torch") is None:
            return
        import torch
    if torch.cuda.is_available():
        torch.cuda.init()


class Engine:
    """A libeigenface context bound to one HIP device."""

    def __init__(self, device: int = 0):
        self._lib = N.lib()
        _init_torch_first()
        h = C.c_void_p()
        rc = self._lib.ef_create(int(device), C.byref(h))
        if rc != N.EF_OK:
            raise N.EigenfaceError(rc, f"ef_create(device={device}) failed (no usable HIP device?)")
        self._h = h
        self.device = int(device)
        self._chk(self._lib.ef_set_option(h, N.EF_OPT_HOST_THREADS, host_cpu_share()))
        # The engine's own stream is a torch pool stream when torch is present: pool streams
        # live as long as the process, so a tensor marked with record_stream (_torch_order)
        # never outlives the stream it was recorded on.  A stream the library created would
        # be destroyed by close() while such a tensor, freed later, still records an event
        # on it (a host crash at free time).
        self._pool_stream = None
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            self._pool_stream = torch.cuda.Stream(device=self.device)
            self._chk(self._lib.ef_set_stream(h, C.c_void_p(self._pool_stream.cuda_stream)))
        self.model_k = None
        self.model_d = None
        self.gallery_n = 0
        self.gallery_k = None
        # Owner tokens of the resident model / gallery: whoever uploads them last owns them.
        # Callers that cache "my model is resident" (EigenfacePCA, recognize_face_with_model)
        # compare their token with these instead of assuming nobody else replaced it.
        self.model_owner = None
        self.recon_owner = None  # None: no reconstruction state (set_reconstruction)
        self.gallery_owner = None
        self.bank_owner = None  # the ModelBank whose slots the bank holds, if one filled it
        self._bank_k = []
        self._tm = None    # (problems, H, W, problem table) of the prepared localiser
        self._scan = None  # (groups, face height, face width) of the frame scan's plan
        self.scan_owner = None  # the FrameScanner whose plan and localiser are in place, if any

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ef_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown ordering
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        return N.check(self._h, rc)

    def set_stream(self, stream_handle):
        """Launch on an external hipStream_t (int handle, e.g. torch's
        ``current_stream().cuda_stream``; 0 is the default stream)."""
        self._chk(self._lib.ef_set_stream(self._h, C.c_void_p(int(stream_handle) or None)))

    def use_own_stream(self):
        """Back to the engine's own non-blocking stream (its torch pool stream, or the
        library's stream without torch)."""
        if self._pool_stream is not None:
            self.set_stream(self._pool_stream.cuda_stream)
        else:
            self._chk(self._lib.ef_use_own_stream(self._h))

    def synchronize(self):
        self._chk(self._lib.ef_synchronize(self._h))

    def stream_handle(self) -> int:
        """The hipStream_t the engine launches on (0 = the default stream)."""
        s = C.c_void_p()
        self._chk(self._lib.ef_get_stream(self._h, C.byref(s)))
        return int(s.value or 0)

    @contextlib.contextmanager
    def _torch_order(self, *tensors):
        """Stream order of a call on device tensors when the engine runs on its own stream:
        the engine's stream first waits for torch's current stream (the inputs' producers),
        then torch's current stream waits for the engine's (the outputs' consumers), and
        every tensor the call reads or writes — inputs included, e.g. a dtype-converted
        temporary that dies when the wrapper returns — is marked as used on the engine's
        stream, so the caching allocator hands its memory to no other stream before the
        engine's kernels are done.  The mark is made only on streams that live as long as
        the process (the engine's torch pool stream, the default stream): a tensor freed
        after its stream was destroyed would crash the allocator; on a caller's external
        stream (set_stream) inputs are safe to reuse on torch's current stream only.  No
        host wait either way; a no-op when the engine already runs on torch's stream."""
        import torch
        h = self.stream_handle()
        cur = torch.cuda.current_stream(self.device)
        if h == cur.cuda_stream:
            yield
            return
        pool = self._pool_stream
        if pool is not None and h == pool.cuda_stream:
            ext = pool
        else:
            ext = torch.cuda.ExternalStream(h, device=self.device) if h else torch.cuda.default_stream(self.device)
        ext.wait_stream(cur)
        yield
        cur.wait_stream(ext)
        if ext is pool or not h:
            for t in tensors:
                if t is not None:
                    t.record_stream(ext)

    def trim(self):
        """Free the fit workspaces the context keeps between fits (ef_trim)."""
        self._chk(self._lib.ef_trim(self._h))

    def chol_inv(self, G, tol_rel=1e-13, Li=None):
        """The fit's CholQR factor alone (ef_chol_inv): (Li, info) with Li = L^-1 for
        G = L L^T (1 <= m <= 256).  On a failed pivot info = -(column + 1) and Li is returned
        as given (zeros by default)."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        m = int(G.shape[0])
        L = np.zeros((m, m), np.float64) if Li is None else np.array(Li, dtype=np.float64, order="C", copy=True)
        info = C.c_int32(0)
        self._chk(self._lib.ef_chol_inv(self._h, G.ctypes.data, m, int(G.shape[1]), float(tol_rel), L.ctypes.data,
                                        C.byref(info)))
        return L, int(info.value)

    def set_option(self, option, value):
        """Context tunable (include/eigenface.h EF_OPT_*): "fit_max_iters",
        "fit_fp32_coarse", "cov_slab_bytes", "tm_int64_sums", "haar_ordered", "jpeg_chunk_bits",
        "search_split_bf16", "jpeg_part_files", "fit_chebyshev", "host_threads" (process-wide),
        "search_prefix", "search_topk_cand", "search_prefix_split", "project_split_bf16", "rank_bitmap_bytes" or
        the code."""
        self._chk(self._lib.ef_set_option(self._h, _option(option), int(value)))

    def get_option(self, option):
        v = C.c_int64(0)
        self._chk(self._lib.ef_get_option(self._h, _option(option), C.byref(v)))
        return int(v.value)

    def search_stats(self):
        """(probes, proven by the prefix scan, sent to the full-k scan, guard skipped) of the
        most recent search (ef_search_stats); synchronises the stream."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.ef_search_stats(self._h, out))
        return tuple(int(v) for v in out)

    def search_screen_stats(self):
        """(probes screened, proven by the screen, screen's guard skipped it) of the most recent
        search (ef_prefix_screen_stats); synchronises the stream."""
        out = (C.c_int64 * 3)()
        self._chk(self._lib.ef_prefix_screen_stats(self._h, out))
        return tuple(int(v) for v in out)

    # --------------------------------------------------------------- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        """A fresh RCCL unique id (rank 0 creates it; broadcast it to the other ranks)."""
        buf = C.create_string_buffer(N.EF_UNIQUE_ID_BYTES)
        rc = N.lib().ef_comm_unique_id(buf)
        if rc != N.EF_OK:
            raise N.EigenfaceError(rc, "ef_comm_unique_id failed (RCCL unavailable?)")
        return bytes(buf.raw)

    def comm_init(self, nranks: int, rank: int, unique_id: bytes):
        """Attach an in-library RCCL communicator (ef_comm_init): from now on search /
        recognize return the global result over the row-sharded gallery."""
        if len(unique_id) != N.EF_UNIQUE_ID_BYTES:
            raise ValueError("unique_id must be EF_UNIQUE_ID_BYTES bytes")
        buf = C.create_string_buffer(bytes(unique_id), N.EF_UNIQUE_ID_BYTES)
        self._chk(self._lib.ef_comm_init(self._h, int(nranks), int(rank), buf))

    def comm_destroy(self):
        self._chk(self._lib.ef_comm_destroy(self._h))

    def comm_info(self):
        n, r = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.ef_comm_info(self._h, C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    # ------------------------------------------------------------------------ fit
    @staticmethod
    def _fit_input(X):
        """(array, pointer, EF dtype, on device) of fit input: uint8 pixels (exact integer
        kernels) or float32 / float64 data (fp64 loaders; include/eigenface.h ef_fit_ex)."""
        if _is_dev(X):
            import torch
            codes = {torch.uint8: N.EF_U8, torch.float32: N.EF_F32, torch.float64: N.EF_F64}
            if X.dtype not in codes:
                raise TypeError(f"fit input must be uint8, float32 or float64, got {X.dtype}")
            x, xp = _dev(X, X.dtype)
            return x, xp, codes[X.dtype], True
        a = np.asarray(X)
        if a.dtype == np.uint8:
            code, dt = N.EF_U8, np.uint8
        elif a.dtype == np.float32:
            code, dt = N.EF_F32, np.float32
        else:
            code, dt = N.EF_F64, np.float64
        x, xp = _host(a, dt)
        return x, xp, code, False

    def fit(self, X, n_components: int, standardize: bool = False, projection: bool = True) -> FitResult:
        """GPU eigenfaces fit of faces X (n x d); see include/eigenface.h ef_fit / ef_fit_ex.

        X is uint8 pixels, or float32 / float64 data (e.g. ManualStandardScaler output,
        scripts/manual/train-v2.py:194-197).  It may be a host array or a device torch
        tensor; for a device X the outputs stay on the device (float64 torch tensors,
        EF_MEM_DEVICE)."""
        x, xp, xdt, dev = self._fit_input(X)
        if dev:
            import torch
        if x.ndim != 2:
            raise ValueError("X must be 2-D (n_samples, n_pixels)")
        n, d = (int(v) for v in x.shape)
        k = int(n_components)
        kk = min(k, n if n < d else d)
        if dev:
            def alloc(*shape):
                return torch.empty(shape, dtype=torch.float64, device=x.device)

            def ptr(a):
                return a.data_ptr()
        else:
            def alloc(*shape):
                return np.empty(shape)

            def ptr(a):
                return a.ctypes.data
        mean, var, scale = alloc(d), alloc(d), alloc(d)
        comps, eig = alloc(kk, d), alloc(kk)
        proj = alloc(n, kk) if projection else None
        tv = alloc(1)
        k_out = C.c_int32(0)
        it = C.c_int32(0)
        flags = (N.EF_FIT_STANDARDIZE if standardize else 0) | (N.EF_MEM_DEVICE if dev else 0)
        with (self._torch_order(x, mean, var, scale, comps, eig, proj, tv) if dev else contextlib.nullcontext()):
            self._chk(self._lib.ef_fit_ex(
                self._h, xp, xdt, n, d, k, flags, ptr(mean), ptr(var), ptr(scale), ptr(comps), ptr(eig),
                ptr(proj) if proj is not None else None, ptr(tv), C.byref(k_out), C.byref(it)))
        if dev:
            self.synchronize()
        return FitResult(mean, var, scale, comps, eig, proj, float(tv[0]), int(k_out.value), int(it.value))

    def colstats(self, X):
        """Column mean and population variance (float64) of X (n x d, uint8 / float32 /
        float64; ef_colstats): np.mean / np.var(axis=0) on the GPU — exact integer sums for
        uint8, two-pass fp64 for floats.  Host input -> numpy, device input -> tensors."""
        x, xp, xdt, dev = self._fit_input(X)
        if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("X must be 2-D (n_samples >= 1, n_features >= 1)")
        n, d = (int(v) for v in x.shape)
        if dev:
            import torch
            mean = torch.empty(d, dtype=torch.float64, device=x.device)
            var = torch.empty(d, dtype=torch.float64, device=x.device)
            with self._torch_order(x, mean, var):
                self._chk(self._lib.ef_colstats(self._h, xp, xdt, n, d, N.EF_MEM_DEVICE, mean.data_ptr(),
                                                var.data_ptr()))
            self.synchronize()
            return mean, var
        mean, var = np.empty(d), np.empty(d)
        self._chk(self._lib.ef_colstats(self._h, xp, xdt, n, d, 0, mean.ctypes.data, var.ctypes.data))
        return mean, var

    # ------------------------------------------------------- Fisher discriminant
    def _lda_input(self, F, labels, n_classes):
        """(features, pointer, EF dtype, int32 labels, pointer, classes, C, on device): float32 /
        float64 features (n, k) with one label per row.  With ``n_classes`` None the labels may
        be any integers and are mapped to 0..C-1 by value (np.unique; ``classes`` holds the
        values); else they are taken as they are, so that empty classes keep their rows."""
        f, fp, fdt, dev = self._fit_input(F)
        if fdt == N.EF_U8:
            raise TypeError("features must be float32 or float64")
        if f.ndim != 2 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("features must be 2-D (n >= 1, k >= 1)")
        n = int(f.shape[0])
        if dev:
            import torch
            lab = labels if _is_dev(labels) else torch.as_tensor(np.asarray(labels), device=f.device)
            if lab.ndim != 1 or lab.shape[0] != n:
                raise ValueError(f"labels must be ({n},), got {tuple(lab.shape)}")
            if n_classes is None:
                classes, lab = torch.unique(lab, return_inverse=True)
                n_classes = int(classes.shape[0])
            else:
                classes = torch.arange(int(n_classes), device=f.device)
            lab = lab.to(torch.int32).contiguous()
            return f, fp, fdt, lab, lab.data_ptr(), classes, int(n_classes), True
        lab = np.asarray(labels)
        if lab.ndim != 1 or lab.shape[0] != n:
            raise ValueError(f"labels must be ({n},), got {lab.shape}")
        if n_classes is None:
            classes, lab = np.unique(lab, return_inverse=True)
            n_classes = len(classes)
        else:
            classes = np.arange(int(n_classes))
            # a value int32 cannot hold is out of range whatever n_classes is
            lab = np.clip(lab, -1, np.iinfo(np.int32).max)
        lab, lp = _host(lab.reshape(-1), np.int32)
        return f, fp, fdt, lab, lp, classes, int(n_classes), False

    def lda_scatter(self, F, labels, n_classes=None):
        """Class statistics of labelled features (ef_lda_scatter), float64: a dict with
        ``counts`` (C,) int64, ``mean`` (k,), ``class_means`` (C, k), ``Sw`` and ``Sb`` (k, k) and
        ``classes`` (the label value of each class).  Labels are mapped to 0..C-1 by value
        unless ``n_classes`` is given (then they must lie in [0, n_classes), and a class
        without rows is empty).  Host arrays in -> NumPy out, device tensors in -> tensors out."""
        f, fp, fdt, lab, lp, classes, C_, dev = self._lda_input(F, labels, n_classes)
        n, k = (int(v) for v in f.shape)
        device = f.device if dev else None
        cnt, mean, cm = _empty(C_, np.int64, device), _empty(k, np.float64, device), _empty((C_, k), np.float64, device)
        sw, sb = _empty((k, k), np.float64, device), _empty((k, k), np.float64, device)
        with self._order(dev, f, lab, cnt, mean, cm, sw, sb):
            self._chk(self._lib.ef_lda_scatter(self._h, fp, fdt, n, k, lp, C_, _ptr(cnt), _ptr(mean), _ptr(cm), _ptr(sw),
                                               _ptr(sb), N.EF_MEM_DEVICE if dev else 0))
        return {"counts": cnt, "mean": mean, "class_means": cm, "Sw": sw, "Sb": sb, "classes": classes}

    def lda_fit(self, F, labels, n_components=None, shrinkage=0.0, n_classes=None) -> "LdaResult":
        """The Fisher discriminant of labelled features (ef_lda_fit; conventions in
        include/eigenface.h): ``scalings`` (k, m) with A^T (Sw_g / (n - C)) A = I, the
        generalised ``eigenvalues`` (m,) descending, ``mean`` (k,), ``class_means`` (C, k) and
        ``classes``.  ``n_components`` defaults to min(k, C - 1) over the non-empty classes.
        Host arrays in -> NumPy out, device tensors in -> tensors out."""
        f, fp, fdt, lab, lp, classes, C_, dev = self._lda_input(F, labels, n_classes)
        n, k = (int(v) for v in f.shape)
        if n_components is None:
            present = int(lab.unique().numel()) if dev else len(np.unique(lab))
            n_components = max(1, min(k, present - 1))
        m = int(n_components)
        if m < 1:
            raise ValueError("n_components must be >= 1")
        device = f.device if dev else None
        A, ev = _empty((k, m), np.float64, device), _empty(m, np.float64, device)
        mean, cm = _empty(k, np.float64, device), _empty((C_, k), np.float64, device)
        with self._order(dev, f, lab, A, ev, mean, cm):
            self._chk(self._lib.ef_lda_fit(self._h, fp, fdt, n, k, lp, C_, m, float(shrinkage), _ptr(A), _ptr(ev),
                                           _ptr(mean), _ptr(cm), N.EF_MEM_DEVICE if dev else 0))
        return LdaResult(A, ev, mean, cm, classes)

    # --------------------------------------------------------- sample-sharded fit
    def fit_shard_stats(self, X):
        """ef_fit_shard_stats: the exact integer pieces of this rank's uint8 rows X (n x d) —
        (sum x [d], sum x^2 [d], X'^T X' [d, d] with X' = X - 128, upper 64-blocks exact) as
        int64 arrays: torch tensors on X's device for a device X, numpy otherwise.  Summed
        over ranks they are the pieces of the whole set (distributed.sharded_fit)."""
        x, xp, xdt, dev = self._fit_input(X)
        if xdt != N.EF_U8 or x.ndim != 2:
            raise TypeError("fit_shard_stats takes 2-D uint8 pixels")
        n, d = (int(v) for v in x.shape)
        if dev:
            import torch
            s1 = torch.empty(d, dtype=torch.int64, device=x.device)
            s2 = torch.empty(d, dtype=torch.int64, device=x.device)
            cr = torch.empty((d, d), dtype=torch.int64, device=x.device)
            with self._torch_order(x, s1, s2, cr):
                self._chk(self._lib.ef_fit_shard_stats(self._h, xp, n, d, s1.data_ptr(), s2.data_ptr(),
                                                       cr.data_ptr(), N.EF_MEM_DEVICE))
            return s1, s2, cr
        s1, s2 = np.empty(d, np.int64), np.empty(d, np.int64)
        cr = np.empty((d, d), np.int64)
        self._chk(self._lib.ef_fit_shard_stats(self._h, xp, n, d, s1.ctypes.data, s2.ctypes.data, cr.ctypes.data, 0))
        return s1, s2, cr

    def fit_from_stats(self, sums, sumsqs, cross, n_total: int, n_components: int, standardize: bool = False) -> FitResult:
        """ef_fit_from_stats: the fit (covariance path, n_total >= d) from the pieces of
        fit_shard_stats summed over every rank — equal to fit() on the concatenated rows bit
        for bit (projection None: see fit_transform_rows).  Device pieces give device
        (float64 torch) outputs."""
        if _is_dev(sums):
            import torch
            s1, p1 = _dev(sums, torch.int64)
            s2, p2 = _dev(sumsqs, torch.int64)
            cr, p3 = _dev(cross, torch.int64)
            d = int(s1.shape[0])
            kk = min(int(n_components), d)

            def alloc(*shape):
                return torch.empty(shape, dtype=torch.float64, device=s1.device)

            def ptr(a):
                return a.data_ptr()
            flags = N.EF_MEM_DEVICE
        else:
            s1, p1 = _host(np.asarray(sums), np.int64)
            s2, p2 = _host(np.asarray(sumsqs), np.int64)
            cr, p3 = _host(np.asarray(cross), np.int64)
            d = int(s1.shape[0])
            kk = min(int(n_components), d)

            def alloc(*shape):
                return np.empty(shape)

            def ptr(a):
                return a.ctypes.data
            flags = 0
        if tuple(cr.shape) != (d, d) or tuple(s2.shape) != (d,):
            raise ValueError(f"pieces must be sum[{d}], sumsq[{d}], cross[{d}, {d}]")
        mean, var, scale = alloc(d), alloc(d), alloc(d)
        comps, eig, tv = alloc(kk, d), alloc(kk), alloc(1)
        k_out, it = C.c_int32(0), C.c_int32(0)
        flags |= N.EF_FIT_STANDARDIZE if standardize else 0
        ctx = self._torch_order(s1, s2, cr, mean, var, scale, comps, eig, tv) if flags & N.EF_MEM_DEVICE \
            else contextlib.nullcontext()
        with ctx:
            self._chk(self._lib.ef_fit_from_stats(self._h, p1, p2, p3, int(n_total), d, int(n_components), flags,
                                                  ptr(mean), ptr(var), ptr(scale), ptr(comps), ptr(eig), ptr(tv),
                                                  C.byref(k_out), C.byref(it)))
        if flags & N.EF_MEM_DEVICE:
            self.synchronize()
        return FitResult(mean, var, scale, comps, eig, None, float(tv[0]), int(k_out.value), int(it.value))

    def fit_transform_rows(self, X, result: FitResult, standardize: bool = False):
        """ef_fit_transform: the training projection of uint8 rows X with a fitted model —
        the rows fit()'s projection holds for them (the sample-sharded fit projects each
        rank's own rows)."""
        x, xp, xdt, dev = self._fit_input(X)
        if xdt != N.EF_U8 or x.ndim != 2:
            raise TypeError("fit_transform_rows takes 2-D uint8 pixels")
        n, d = (int(v) for v in x.shape)
        k = int(result.k)
        if dev:
            import torch
            mean, pm = _dev(result.mean, torch.float64)
            comps, pc = _dev(result.components, torch.float64)
            sc, ps = _dev(result.scale, torch.float64) if standardize else (None, None)
            out = torch.empty((n, k), dtype=torch.float64, device=x.device)
            with self._torch_order(x, mean, comps, sc, out):
                self._chk(self._lib.ef_fit_transform(self._h, xp, n, d, pm, ps, pc, k, N.EF_MEM_DEVICE,
                                                     out.data_ptr()))
            return out
        mean, pm = _host(np.asarray(result.mean), np.float64)
        comps, pc = _host(np.asarray(result.components), np.float64)
        sc, ps = _host(np.asarray(result.scale), np.float64) if standardize else (None, None)
        out = np.empty((n, k))
        self._chk(self._lib.ef_fit_transform(self._h, xp, n, d, pm, ps, pc, k, 0, out.ctypes.data))
        return out

    # ----------------------------------------------------------------- projection
    def set_model(self, mean, W, precision="fp32", owner=None):
        """Resident recognition model f = (p - mean) . W, W is d x k (k <= 512).

        precision="bf16" projects on bf16 MFMA (BASELINE.json config 5):
        f = (p - round(mean)).bf16(W) - (mean - round(mean)).W, fp32 accumulation;
        features, gallery search and arg-best stay fp32 (fp64-resolved)."""
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        if _is_dev(W):
            import torch
            m, mp = _dev(mean, torch.float32)
            w, wp = _dev(W, torch.float32)
            flags = N.EF_MEM_DEVICE
        else:
            m, mp = _host(mean, np.float32)
            w, wp = _host(W, np.float32)
            flags = 0
        d, k = w.shape
        if m.shape[0] != d:
            raise ValueError("mean and W disagree on d")
        if precision == "bf16":
            flags |= N.EF_MODEL_BF16
        self.model_owner = None  # a failed upload leaves no valid owner
        self.recon_owner = None  # ef_model_set drops the reconstruction state
        self._chk(self._lib.ef_model_set(self._h, mp, wp, d, k, flags))
        if flags:
            self.synchronize()
        self.model_d, self.model_k = int(d), int(k)
        self.model_owner = owner if owner is not None else object()

    def _dev_pixels(self, P):
        """Validated device probe pixels: (b, model_d) uint8 or float32, contiguous."""
        import torch
        if P.dtype not in (torch.uint8, torch.float32):
            raise TypeError(f"probe pixels must be uint8 or float32, got {P.dtype}")
        if P.ndim != 2 or P.shape[1] != self.model_d:
            raise ValueError(f"P must be (b, {self.model_d}), got {tuple(P.shape)}")
        p, pp = _dev(P, P.dtype)
        return p, pp, (N.EF_U8 if P.dtype == torch.uint8 else N.EF_F32)

    @staticmethod
    def _dev_out(t, shape, dtype, what):
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)}")
        return t

    def project(self, P, out=None):
        if self.model_k is None:
            raise RuntimeError("no model: call set_model first")
        if _is_dev(P):
            import torch
            p, pp, dtype = self._dev_pixels(P)
            b = p.shape[0]
            if out is None:
                out = torch.empty((b, self.model_k), dtype=torch.float32, device=p.device)
            self._dev_out(out, (b, self.model_k), torch.float32, "out")
            with self._torch_order(p, out):
                self._chk(self._lib.ef_project(self._h, pp, dtype, b, out.data_ptr(), N.EF_MEM_DEVICE))
            return out
        p = np.asarray(P)
        dtype = N.EF_U8 if p.dtype == np.uint8 else N.EF_F32
        p, pp = _host(p, np.uint8 if dtype == N.EF_U8 else np.float32)
        if p.ndim != 2 or p.shape[1] != self.model_d:
            raise ValueError("P must be (b, d)")
        b = p.shape[0]
        f = np.empty((b, self.model_k), dtype=np.float32)
        self._chk(self._lib.ef_project(self._h, pp, dtype, b, f.ctypes.data, 0))
        return f

    # ------------------------------------------------------------- reconstruction
    def set_reconstruction(self, R, weight=None, owner=None):
        """The way back for the resident model: x^ = mean + f . R with R (k x d) and an optional
        per-pixel weight (d,) of the residual (ef_recon_set).  manual_pca models: R =
        eigenfaces^T; standardised models (W = diag(1/sigma) V^T): R = V diag(sigma), weight =
        1/sigma.  A later set_model drops it."""
        if self.model_k is None:
            raise RuntimeError("no model: call set_model first")
        if _is_dev(R):
            import torch
            r, rp = _dev(R, torch.float32)
            w, wp = _dev(weight, torch.float32) if weight is not None else (None, None)
            flags = N.EF_MEM_DEVICE
        else:
            r, rp = _host(R, np.float32)
            w, wp = _host(weight, np.float32) if weight is not None else (None, None)
            flags = 0
        if r.ndim != 2:
            raise ValueError("R must be 2-D (k, d)")
        k, d = (int(v) for v in r.shape)
        if w is not None and tuple(w.shape) != (d,):
            raise ValueError("weight and R disagree on d")
        self.recon_owner = None  # a failed upload leaves none
        self._chk(self._lib.ef_recon_set(self._h, rp, wp, d, k, flags))
        self.recon_owner = owner if owner is not None else object()

    def reconstruct(self, F, dtype="float32", out=None):
        """x^ = mean + F . R for features F (b, k): float32, or uint8 (clamped to [0, 255], then
        rounded half to even) (ef_reconstruct).  Device F gives a device result (``out``
        optional); host F a NumPy array."""
        if self.model_k is None:
            raise RuntimeError("no model: call set_model first")
        if dtype not in ("float32", "uint8"):
            raise ValueError("dtype must be 'float32' or 'uint8'")
        code = N.EF_U8 if dtype == "uint8" else N.EF_F32
        if _is_dev(F):
            import torch
            f, fp = _dev(F, torch.float32)
            if f.ndim != 2 or f.shape[1] != self.model_k:
                raise ValueError(f"F must be (b, {self.model_k}), got {tuple(f.shape)}")
            b = f.shape[0]
            tdt = torch.uint8 if dtype == "uint8" else torch.float32
            if out is None:
                out = torch.empty((b, self.model_d), dtype=tdt, device=f.device)
            self._dev_out(out, (b, self.model_d), tdt, "out")
            with self._torch_order(f, out):
                self._chk(self._lib.ef_reconstruct(self._h, fp, b, code, out.data_ptr(), N.EF_MEM_DEVICE))
            return out
        f, fp = _host(F, np.float32)
        if f.ndim != 2 or f.shape[1] != self.model_k:
            raise ValueError("F must be (b, k)")
        b = f.shape[0]
        ndt = np.uint8 if dtype == "uint8" else np.float32
        if out is None:
            out = np.empty((b, self.model_d), dtype=ndt)
        elif not (isinstance(out, np.ndarray) and out.dtype == ndt and out.shape == (b, self.model_d)
                  and out.flags.c_contiguous):
            raise ValueError(f"out must be a contiguous {dtype} array of shape {(b, self.model_d)}")
        self._chk(self._lib.ef_reconstruct(self._h, fp, b, code, out.ctypes.data, 0))
        return out

    def face_distance(self, P, return_energy=False, return_features=False, out=None):
        """Squared distance from face space eps^2 = sum_j (s_j (p_j - x^_j))^2 of pixels P (b, d),
        uint8 or float32 (ef_face_distance): projection, reduce and residual in one stream-ordered
        sequence, x^ never written.  Returns eps^2 (b,) float32 and, when asked, the energy
        sum_j (s_j (p_j - mean_j))^2 and the features (exactly ``project(P)``), in that order.
        Device P gives device results; ``out`` is then an optional float32 tensor (b,) for eps^2."""
        if self.model_k is None:
            raise RuntimeError("no model: call set_model first")
        if _is_dev(P):
            import torch
            p, pp, dtype = self._dev_pixels(P)
            b = p.shape[0]
            if out is None:
                out = torch.empty((b,), dtype=torch.float32, device=p.device)
            self._dev_out(out, (b,), torch.float32, "out")
            en = torch.empty((b,), dtype=torch.float32, device=p.device) if return_energy else None
            ft = torch.empty((b, self.model_k), dtype=torch.float32, device=p.device) if return_features else None
            with self._torch_order(p, out, en, ft):
                self._chk(self._lib.ef_face_distance(self._h, pp, dtype, b, out.data_ptr(),
                                                     en.data_ptr() if en is not None else None,
                                                     ft.data_ptr() if ft is not None else None, N.EF_MEM_DEVICE))
        else:
            if out is not None:
                raise ValueError("out= is for device tensors")
            p = np.asarray(P)
            dtype = N.EF_U8 if p.dtype == np.uint8 else N.EF_F32
            p, pp = _host(p, np.uint8 if dtype == N.EF_U8 else np.float32)
            if p.ndim != 2 or p.shape[1] != self.model_d:
                raise ValueError("P must be (b, d)")
            b = p.shape[0]
            out = np.empty((b,), dtype=np.float32)
            en = np.empty((b,), dtype=np.float32) if return_energy else None
            ft = np.empty((b, self.model_k), dtype=np.float32) if return_features else None
            self._chk(self._lib.ef_face_distance(self._h, pp, dtype, b, out.ctypes.data,
                                                 en.ctypes.data if en is not None else None,
                                                 ft.ctypes.data if ft is not None else None, 0))
        res = (out,) + ((en,) if return_energy else ()) + ((ft,) if return_features else ())
        return res[0] if len(res) == 1 else res

    # --------------------------------------------------------------------- search
    def set_gallery(self, G, global_offset: int = 0, owner=None):
        if _is_dev(G):
            import torch
            g, gp = _dev(G, torch.float32)
            flags = N.EF_MEM_DEVICE
        else:
            g, gp = _host(G, np.float32)
            flags = 0
        if g.ndim != 2:
            raise ValueError("gallery must be 2-D (n, k)")
        n, k = g.shape
        self.gallery_owner = None
        self._chk(self._lib.ef_gallery_set(self._h, gp, n, k, int(global_offset), flags))
        self.gallery_n, self.gallery_k = int(n), int(k)
        self.gallery_owner = owner if owner is not None else object()

    def _probes(self, X, pixels):
        """The probes of a search call as the C side reads them: (array or tensor, pointer,
        dtype code, b, on_device).  Features are float32 (b, gallery_k), pixels uint8 or float32
        (b, model_d); host input is converted to a contiguous array, a device tensor is taken
        as it is (made contiguous).  The C side reads b * width elements from the pointer, so a
        narrower or 1-D input, which would be read past its end, is refused here."""
        dev = _is_dev(X)
        if pixels:
            if dev:
                x, xp, dtype = self._dev_pixels(X)
            else:
                x = np.asarray(X)
                dtype = N.EF_U8 if x.dtype == np.uint8 else N.EF_F32
                x, xp = _host(x, np.uint8 if dtype == N.EF_U8 else np.float32)
            want, name = self.model_d, "P"
        else:
            if dev:
                import torch
                x, xp = _dev(X, torch.float32)
            else:
                x, xp = _host(X, np.float32)
            dtype, want, name = N.EF_F32, self.gallery_k, "Q"
        if x.ndim != 2 or x.shape[1] != want:
            raise ValueError(f"{name} must be (b, {want}), got {tuple(x.shape)}")
        return x, xp, dtype, x.shape[0], dev

    def _result(self, x, dev, out, shape, records, what):
        """The output of a call on probes x and its pointer: for device input the caller's
        int64 tensor (validated) or a new one, records as (.., 3) int64; for host input a new
        array of int64 keys or N.MATCH_DTYPE records."""
        if not dev:
            res = np.empty(shape, dtype=N.MATCH_DTYPE if records else np.int64)
            return res, res.ctypes.data
        import torch
        if records:
            shape = shape + (3,)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=x.device)
        self._dev_out(out, shape, torch.int64, what)
        return out, out.data_ptr()

    def _order(self, dev, *tensors):
        return self._torch_order(*tensors) if dev else contextlib.nullcontext()

    def search_keys(self, Q, metric="l2", keys=None):
        """Packed keys (int64) of the best gallery row per probe."""
        mt = _metric(metric)
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        q, qp, _, b, dev = self._probes(Q, pixels=False)
        keys, kp = self._result(q, dev, keys, (b,), False, "keys")
        with self._order(dev, q, keys):
            self._chk(self._lib.ef_search(self._h, qp, b, mt, kp, N.EF_MEM_DEVICE if dev else 0))
        return keys

    def search(self, Q, metric="l2"):
        """Return (idx int64, best float32): L2 -> squared distance, cosine -> similarity."""
        keys = self.search_keys(Q, metric)
        if _is_dev(keys):
            keys = keys.cpu().numpy()
        return decode_keys(keys, metric)

    def recognize_keys(self, P, metric="l2", keys=None, feats=None):
        """Fused projection + search (device or host)."""
        mt = _metric(metric)
        if self.model_k is None or self.gallery_k is None:
            raise RuntimeError("recognize needs a model and a gallery")
        p, pp, dtype, b, dev = self._probes(P, pixels=True)
        keys, kp = self._result(p, dev, keys, (b,), False, "keys")
        fp = None
        if dev and feats is not None:
            import torch
            fp = self._dev_out(feats, (b, self.model_k), torch.float32, "feats").data_ptr()
        elif feats is not None:
            if not (isinstance(feats, np.ndarray) and feats.dtype == np.float32 and feats.shape == (b, self.model_k)
                    and feats.flags.c_contiguous):
                raise ValueError(f"feats must be a contiguous float32 array of shape {(b, self.model_k)}")
            fp = feats.ctypes.data
        with self._order(dev, p, keys, feats):
            self._chk(self._lib.ef_recognize(self._h, pp, dtype, b, mt, kp, fp, N.EF_MEM_DEVICE if dev else 0))
        return keys

    # ------------------------------------------------------- exact match records
    def search_matches(self, Q, metric="l2", out=None):
        """ef_search_matches: per-probe (fp64 score, scale, key) records (numpy structured
        array of N.MATCH_DTYPE on the host; an (b, 3) int64 tensor for device input)."""
        return self._matches(Q, metric, out, search=True)

    def recognize_matches(self, P, metric="l2", out=None):
        """ef_recognize_matches: projection + search, returning match records."""
        return self._matches(P, metric, out, search=False)

    def _matches(self, X, metric, out, search):
        mt = _metric(metric)
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        if not search and self.model_k is None:
            raise RuntimeError("recognize needs a model and a gallery")
        x, xp, dtype, b, dev = self._probes(X, pixels=not search)
        out, op = self._result(x, dev, out, (b,), True, "out")
        flags = N.EF_MEM_DEVICE if dev else 0
        with self._order(dev, x, out):
            if search:
                self._chk(self._lib.ef_search_matches(self._h, xp, b, mt, op, flags))
            else:
                self._chk(self._lib.ef_recognize_matches(self._h, xp, dtype, b, mt, op, None, flags))
        return out

    def merge_matches(self, parts, b, keys=None):
        """Device merge (ef_matches_merge, EF_MEM_DEVICE) of gathered records: ``parts`` is
        an (nparts*b, 3) int64 tensor (part-major) -> int64 keys[b]."""
        import torch
        b = int(b)
        if not (isinstance(parts, torch.Tensor) and parts.is_cuda):
            raise TypeError("parts must be a device tensor (use merge_matches_host for host records)")
        if parts.dtype != torch.int64 or parts.ndim != 2 or parts.shape[1] != 3 or not parts.is_contiguous():
            raise ValueError(f"parts must be a contiguous (nparts*b, 3) int64 tensor, got "
                             f"{parts.dtype} {tuple(parts.shape)}")
        if b < 0 or (b and parts.shape[0] % b) or (b == 0 and parts.shape[0]):
            raise ValueError(f"parts has {parts.shape[0]} records, not a multiple of b = {b}")
        nparts = parts.shape[0] // b if b else 0
        if keys is None:
            keys = torch.empty(b, dtype=torch.int64, device=parts.device)
        elif not (keys.dtype == torch.int64 and tuple(keys.shape) == (b,) and keys.is_contiguous()
                  and keys.device == parts.device):
            raise ValueError(f"keys must be a contiguous int64 tensor of shape ({b},) on {parts.device}")
        if b:
            with self._torch_order(parts, keys):
                self._chk(self._lib.ef_matches_merge(self._h, parts.data_ptr(), nparts, b, keys.data_ptr(), None,
                                                     N.EF_MEM_DEVICE))
        return keys

    # ---------------------------------------------------------- labelled search
    def set_gallery_labels(self, labels):
        """ef_gallery_labels: one int32 label per resident gallery row (a host array or a
        device tensor); ``None`` drops the labels.  set_gallery drops them too."""
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        if labels is None:
            self._chk(self._lib.ef_gallery_labels(self._h, None, 0, 0))
            return
        if _is_dev(labels):
            import torch
            lab, lp = _dev(labels, torch.int32)
            flags = N.EF_MEM_DEVICE
        else:
            lab, lp = _host(labels, np.int32)
            flags = 0
        if lab.ndim != 1:
            raise ValueError("labels must be 1-D (n,)")
        with self._order(flags != 0, lab):
            self._chk(self._lib.ef_gallery_labels(self._h, lp, lab.shape[0], flags))

    def _labelled(self, Q, probe_labels, relation, exclude_rows, metric, out, records):
        mt = _metric(metric)
        rel = _RELATIONS[relation.lower()] if isinstance(relation, str) else int(relation)
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        q, qp, _, b, dev = self._probes(Q, pixels=False)
        pl, plp = _per_probe(probe_labels, np.int32, "probe_labels", q, dev)
        ex, exp = _per_probe(exclude_rows, np.int64, "exclude_rows", q, dev)
        if pl is None and rel != N.EF_LABEL_ANY:
            raise ValueError("probe_labels are required for the relations 'same' and 'other'")
        out, op = self._result(q, dev, out, (b,), records, "out" if records else "keys")
        with self._order(dev, q, pl, ex, out):
            self._chk(self._lib.ef_search_labelled(self._h, qp, b, mt, rel, plp, exp, None if records else op,
                                                   op if records else None, N.EF_MEM_DEVICE if dev else 0))
        return out

    def search_labelled_keys(self, Q, probe_labels, relation="same", exclude_rows=None, metric="l2", keys=None):
        """ef_search_labelled: per probe the packed key search_keys would return on the
        sub-gallery of the rows whose label stands in ``relation`` ("same", "other", "any") to
        the probe's and whose global index is not ``exclude_rows[p]`` (negative: nothing
        excluded); EF_KEY_NONE when no row qualifies.  Host arrays in, a host array out; device
        tensors in, a device tensor out (stream-ordered, as search_keys)."""
        return self._labelled(Q, probe_labels, relation, exclude_rows, metric, keys, False)

    def search_labelled(self, Q, probe_labels, relation="same", exclude_rows=None, metric="l2"):
        """(idx int64, best float32) of search_labelled_keys; (-1, NaN) where no row qualifies."""
        keys = self.search_labelled_keys(Q, probe_labels, relation, exclude_rows, metric)
        if _is_dev(keys):
            keys = keys.cpu().numpy()
        return decode_keys(keys, metric)

    def search_labelled_matches(self, Q, probe_labels, relation="same", exclude_rows=None, metric="l2", out=None):
        """The match records of the labelled search (as search_matches returns them): shards
        searched one by one merge with merge_matches / merge_matches_host unchanged."""
        return self._labelled(Q, probe_labels, relation, exclude_rows, metric, out, True)

    # ------------------------------------------------------------- score census
    def score_census(self, Q, probe_labels, exclude_rows=None, metric="cosine", nbins=256, range=(-1.0, 1.0),
                     counts=None):
        """ef_score_census: histograms of all genuine (row 0) and all impostor (row 1) pair scores
        of the probes against the labelled resident gallery, an int64 array (2, nbins + 3): slot 0
        the scores below ``range[0]``, slots 1 .. nbins the bins, slot nbins + 1 the scores at or
        above ``range[1]``, slot nbins + 2 the pairs whose score is not finite.  The pair of probe
        p with the row of global index ``exclude_rows[p]`` is left out (negative: nothing).  Host
        arrays in, a host array out; device tensors in, a device tensor out (stream-ordered, as
        search_labelled_keys; ``counts``: the caller's tensor)."""
        mt = _metric(metric)
        nbins = int(nbins)
        if not 1 <= nbins <= N.EF_CENSUS_MAX_BINS:
            raise ValueError(f"nbins must be 1 .. {N.EF_CENSUS_MAX_BINS}, got {nbins}")
        lo, hi = (float(np.float32(v)) for v in range)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError(f"range must be finite (lo, hi) with lo < hi in float32, got {tuple(range)}")
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        if probe_labels is None:
            raise ValueError("probe_labels are required")
        q, qp, _, b, dev = self._probes(Q, pixels=False)
        pl, plp = _per_probe(probe_labels, np.int32, "probe_labels", q, dev)
        ex, exp = _per_probe(exclude_rows, np.int64, "exclude_rows", q, dev)
        shape = (2, nbins + 3)
        if dev:
            import torch
            if counts is None:
                counts = torch.empty(shape, dtype=torch.int64, device=q.device)
            self._dev_out(counts, shape, torch.int64, "counts")
            cp = counts.data_ptr()
        else:
            if counts is not None:
                raise ValueError("counts is for device input; host input returns a new array")
            counts = np.empty(shape, np.int64)
            cp = counts.ctypes.data
        with self._order(dev, q, pl, ex, counts):
            self._chk(self._lib.ef_score_census(self._h, qp, b, mt, plp, exp, lo, hi, nbins, cp,
                                                N.EF_MEM_DEVICE if dev else 0))
        return counts

    # ------------------------------------------------------- gallery clustering
    def cluster_gallery(self, threshold, metric="l2", min_samples=1, degree=False, labels=None):
        """ef_gallery_cluster: group the resident gallery's rows by identity without labels.  Rows
        i != j are linked when their fp64 squared distance is <= ``threshold`` (l2) or their fp64
        cosine similarity is >= ``threshold`` (cosine), every edge decided as in fp64; the result
        is the connected components, numbered by their lowest member row.  ``min_samples`` > 1
        adds DBSCAN's density floor (noise rows get -1).

        Returns ``(labels int32 (n,), degree int32 (n,) or None, info int64 (4,))`` with info =
        (clusters, noise rows, linked unordered pairs, pairs settled in fp64).  Host outputs are
        numpy arrays.  With ``labels`` a caller's int32 device tensor of shape (n,) (and ``degree``
        either a bool or such a tensor) the outputs are device tensors and the call is
        stream-ordered without a host wait; bit EF_CLUSTER_UNCONVERGED of info[3] then reports
        what a host call raises."""
        mt = _metric(metric)
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        n = self.gallery_n
        dev = labels is not None
        if dev:
            import torch
            if not _is_dev(labels):
                raise TypeError("labels must be a device tensor (host outputs are returned as new arrays)")
            self._dev_out(labels, (n,), torch.int32, "labels")
            if _is_dev(degree):
                self._dev_out(degree, (n,), torch.int32, "degree")
            elif degree is not None and not isinstance(degree, (bool, np.bool_)):
                raise TypeError("degree must be a bool or an int32 device tensor")
            else:
                degree = torch.empty(n, dtype=torch.int32, device=labels.device) if degree else None
            info = torch.empty(4, dtype=torch.int64, device=labels.device)
        else:
            if _is_dev(degree):
                raise ValueError("a degree tensor needs a labels tensor too")
            labels = np.empty(n, np.int32)
            degree = np.empty(n, np.int32) if degree else None
            info = np.zeros(4, np.int64)
        with self._order(dev, labels, degree, info):
            self._chk(self._lib.ef_gallery_cluster(self._h, mt, threshold, int(min_samples), _ptr(labels), _ptr(degree),
                                                   _ptr(info), N.EF_MEM_DEVICE if dev else 0))
        return labels, degree, info

    # ------------------------------------------------------------- range search
    def _range_call(self, q, qp, b, dev, mt, threshold, ex, exp, cap, rows, scores):
        """One ef_search_range on prepared probes: (lims, info); rows / scores of ``cap`` entries are
        the caller's (None with cap 0: the count-only form)."""
        device = q.device if dev else None
        lims = _empty(b + 1, np.int64, device)
        info = _empty(4, np.int64, device)
        with self._order(dev, q, ex, lims, rows, scores, info):
            self._chk(self._lib.ef_search_range(self._h, qp, b, mt, threshold, exp, _ptr(lims), _ptr(rows),
                                                _ptr(scores), cap, _ptr(info), N.EF_MEM_DEVICE if dev else 0))
        return lims, info

    def _range_args(self, Q, threshold, metric, exclude_rows):
        mt = _metric(metric)
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        q, qp, _, b, dev = self._probes(Q, pixels=False)
        ex, exp = _per_probe(exclude_rows, np.int64, "exclude_rows", q, dev)
        return mt, threshold, q, qp, b, dev, ex, exp

    def search_range(self, Q, threshold, metric="l2", exclude_rows=None, max_results=None, out=None):
        """ef_search_range: for each probe ALL resident rows within ``threshold`` (fp64 squared
        distance <= threshold for l2, fp64 cosine similarity >= threshold for cosine, every
        membership decided as in fp64), as a ``RangeResult``: ``lims`` int64 (b + 1,), ``rows`` int64
        global row indices ascending inside each probe's segment, ``scores`` float32, ``info`` int64
        (4,) = (hits, pairs settled in fp64, hits not written, 0).  The pair of probe p with the row
        of global index ``exclude_rows[p]`` is left out (negative: nothing).

        Host arrays in, numpy arrays out; device tensors in, device tensors out, stream-ordered as
        score_census.  ``max_results`` is the capacity of rows / scores (``out``: the caller's
        (rows, scores) device tensors, whose length is then the capacity): one call that never
        waits on the device route; a probe's segment is written only when it fits whole
        (``lims[p + 1] <= capacity``), and ``complete`` of a device result is None until the caller
        reads ``lims[-1]``.  With ``max_results`` None the capacity starts at 16 hits per probe and
        at least 65 536 (a policy, not a measurement); when ``lims[-1]`` exceeds it the call is made
        once more with exactly ``lims[-1]``.  Reading ``lims[-1]`` is one host wait on the device
        route, the only one."""
        from .neighbors import RangeResult
        mt, threshold, q, qp, b, dev, ex, exp = self._range_args(Q, threshold, metric, exclude_rows)
        device = q.device if dev else None
        if out is not None:
            if not dev:
                raise ValueError("out is for device input; host input returns new arrays")
            import torch
            rows, scores = out
            cap = int(rows.shape[0])
            self._dev_out(rows, (cap,), torch.int64, "out[0] (rows)")
            self._dev_out(scores, (cap,), torch.float32, "out[1] (scores)")
        else:
            cap = max(16 * b, 65536) if max_results is None else int(max_results)
            if cap < 0:
                raise ValueError("max_results must not be negative")
            rows, scores = _empty(cap, np.int64, device), _empty(cap, np.float32, device)
        lims, info = self._range_call(q, qp, b, dev, mt, threshold, ex, exp, cap, rows, scores)
        if max_results is None and out is None:
            total = int(lims[-1])  # the documented wait of the device route
            if total > cap:
                cap = total
                rows, scores = _empty(cap, np.int64, device), _empty(cap, np.float32, device)
                lims, info = self._range_call(q, qp, b, dev, mt, threshold, ex, exp, cap, rows, scores)
            rows, scores = rows[:total], scores[:total]
        elif not dev:
            written = int(info[0] - info[2]) if cap > 0 else 0
            rows, scores = rows[:written], scores[:written]
        return RangeResult(lims, rows, scores, info, "l2" if mt == N.EF_METRIC_L2 else "cosine", cap)

    def search_range_counts(self, Q, threshold, metric="l2", exclude_rows=None):
        """The count-only form of search_range (one pass of the kernel, nothing but ``lims`` and
        ``info`` written): ``(counts int64 (b,), info int64 (4,))`` with counts = the hits of each
        probe and info[0] their total.  Host arrays in, numpy out; device tensors in, device tensors
        out without a host wait."""
        mt, threshold, q, qp, b, dev, ex, exp = self._range_args(Q, threshold, metric, exclude_rows)
        lims, info = self._range_call(q, qp, b, dev, mt, threshold, ex, exp, 0, None, None)
        return lims[1:] - lims[:-1], info

    def recognize_range(self, P, threshold, metric="l2", exclude_rows=None, max_results=None, out=None):
        """Projection of the pixels P (b, d) with the resident model, then search_range on the
        features.  A device input stays on the device."""
        if self.model_k is None or self.gallery_k is None:
            raise RuntimeError("recognize needs a model and a gallery")
        return self.search_range(self.project(P), threshold, metric, exclude_rows, max_results, out)

    # ------------------------------------------------------- identification rank
    def search_rank(self, Q, probe_labels, exclude_rows=None, metric="l2", genuine=None, out=None):
        """ef_search_rank: for each probe the number of OTHER identities with a resident row that
        beats the probe's genuine row (the nearest row of its own label, ``exclude_rows[p]`` left
        out), every comparison decided as in fp64 with the first-index rule on ties.  The
        identification rank is ``better + 1``; ``better`` is -1 for a probe without a genuine row
        (see ``evaluate.cmc_curve``).  The gallery needs labels (set_gallery_labels).

        Returns ``(better int32 (b,), genuine records (b,), info int64 (4,))`` with info = (pairs
        settled in fp64, pieces, distinct labels, 0); the records are those of
        ``search_labelled_matches(.., "same")``.  With ``genuine`` given (records merged over
        shards with merge_matches / merge_matches_host) they are taken as the genuine rows instead
        of searched for: over a gallery sharded by identity the shards' ``better`` add up.

        Host arrays in, numpy arrays out; device tensors in, device tensors out, stream-ordered as
        search_range (``out``: the caller's int32 tensor for ``better``).  The first call after
        set_gallery_labels builds the class map on the host and waits."""
        mt = _metric(metric)
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        if probe_labels is None:
            raise ValueError("probe_labels are required")
        q, qp, _, b, dev = self._probes(Q, pixels=False)
        pl, plp = _per_probe(probe_labels, np.int32, "probe_labels", q, dev)
        ex, exp = _per_probe(exclude_rows, np.int64, "exclude_rows", q, dev)
        device = q.device if dev else None
        flags = N.EF_MEM_DEVICE if dev else 0
        if genuine is None:
            gen, gp = self._result(q, dev, None, (b,), True, "genuine")
        else:
            flags |= N.EF_RANK_GENUINE_GIVEN
            if dev:
                import torch
                if not _is_dev(genuine):
                    raise TypeError("genuine must be a device tensor for device probes")
                gen = self._dev_out(genuine, (b, 3), torch.int64, "genuine")
                gp = gen.data_ptr()
            else:
                gen = np.ascontiguousarray(genuine, dtype=N.MATCH_DTYPE)
                if gen.shape != (b,):
                    raise ValueError(f"genuine must be ({b},) match records, got {gen.shape}")
                gp = gen.ctypes.data
        if out is not None:
            if not dev:
                raise ValueError("out is for device input; host input returns new arrays")
            import torch
            better = self._dev_out(out, (b,), torch.int32, "out")
        else:
            better = _empty(b, np.int32, device)
        info = _empty(4, np.int64, device)
        with self._order(dev, q, pl, ex, gen, better, info):
            self._chk(self._lib.ef_search_rank(self._h, qp, b, mt, plp, exp, gp, _ptr(better), _ptr(info), flags))
        return better, gen, info

    def recognize_rank(self, P, probe_labels, exclude_rows=None, metric="l2", genuine=None, out=None):
        """Projection of the pixels P (b, d) with the resident model, then search_rank on the
        features.  A device input stays on the device."""
        if self.model_k is None or self.gallery_k is None:
            raise RuntimeError("recognize needs a model and a gallery")
        return self.search_rank(self.project(P), probe_labels, exclude_rows, metric, genuine, out)

    # ------------------------------------------------------------- top-m search
    def _topk_m(self, m):
        m = int(m)
        if not 1 <= m <= N.EF_TOPK_MAX:
            raise ValueError(f"m must be 1 .. {N.EF_TOPK_MAX}, got {m}")
        return m

    def _topk(self, X, m, metric, out, kind):
        """The three top-m calls: kind "keys" (ef_search_topk), "matches"
        (ef_search_topk_matches) or "recognize" (ef_recognize_topk)."""
        mt = _metric(metric)
        m = self._topk_m(m)
        if self.gallery_k is None:
            raise RuntimeError("no gallery: call set_gallery first")
        pixels = kind == "recognize"
        if pixels and self.model_k is None:
            raise RuntimeError("recognize needs a model and a gallery")
        x, xp, dtype, b, dev = self._probes(X, pixels)
        out, op = self._result(x, dev, out, (b, m), kind == "matches", "out" if kind == "matches" else "keys")
        flags = N.EF_MEM_DEVICE if dev else 0
        with self._order(dev, x, out):
            if kind == "keys":
                self._chk(self._lib.ef_search_topk(self._h, xp, b, m, mt, op, flags))
            elif kind == "matches":
                self._chk(self._lib.ef_search_topk_matches(self._h, xp, b, m, mt, op, flags))
            else:
                self._chk(self._lib.ef_recognize_topk(self._h, xp, dtype, b, m, mt, op, None, flags))
        return out

    def search_topk_keys(self, Q, m, metric="l2", keys=None):
        """ef_search_topk: packed keys (b, m) int64 of the m best gallery rows per probe, best
        first (rank 0 is search_keys' key; EF_KEY_NONE past the gallery's rows).  Host arrays
        in, a host array out; a device tensor in, a device tensor out (stream-ordered)."""
        return self._topk(Q, m, metric, keys, "keys")

    def search_topk(self, Q, m, metric="l2"):
        """(idx int64 (b, m), best float32 (b, m)) of the m best rows per probe: L2 -> squared
        distance, cosine -> similarity; (-1, NaN) past the gallery's rows."""
        keys = self.search_topk_keys(Q, m, metric)
        return _decode_topk(keys, metric)

    def recognize_topk_keys(self, P, m, metric="l2", keys=None):
        """ef_recognize_topk: projection + top-m search, packed keys (b, m)."""
        return self._topk(P, m, metric, keys, "recognize")

    def recognize_topk(self, P, m, metric="l2"):
        """Project probes P (uint8 / float32 pixels) and return (idx (b, m), best (b, m))."""
        return _decode_topk(self.recognize_topk_keys(P, m, metric), metric)

    def search_topk_matches(self, Q, m, metric="l2", out=None):
        """ef_search_topk_matches: the (fp64 score, scale, key) records of the m best rows per
        probe: a (b, m) array of N.MATCH_DTYPE on the host, a (b, m, 3) int64 tensor for
        device input."""
        return self._topk(Q, m, metric, out, "matches")

    def merge_topk(self, parts, b, m, keys=None):
        """Device merge (ef_matches_merge_topk, EF_MEM_DEVICE) of gathered top-m records:
        ``parts`` is an int64 tensor of nparts * b * m records of 3 words (part-major, any
        shape ending in 3) -> int64 keys (b, m)."""
        import torch
        b, m = int(b), self._topk_m(m)
        if not (isinstance(parts, torch.Tensor) and parts.is_cuda):
            raise TypeError("parts must be a device tensor (use merge_topk_host for host records)")
        if parts.dtype != torch.int64 or parts.ndim < 2 or parts.shape[-1] != 3 or not parts.is_contiguous():
            raise ValueError(f"parts must be a contiguous int64 tensor of records (.., 3), got "
                             f"{parts.dtype} {tuple(parts.shape)}")
        nrec = parts.numel() // 3
        if b < 0 or (b and nrec % (b * m)) or (b == 0 and nrec):
            raise ValueError(f"parts has {nrec} records, not a multiple of b * m = {b * m}")
        nparts = nrec // (b * m) if b else 0
        if keys is None:
            keys = torch.empty((b, m), dtype=torch.int64, device=parts.device)
        elif not (keys.dtype == torch.int64 and tuple(keys.shape) == (b, m) and keys.is_contiguous()
                  and keys.device == parts.device):
            raise ValueError(f"keys must be a contiguous int64 tensor of shape ({b}, {m}) on {parts.device}")
        if b:
            with self._torch_order(parts, keys):
                self._chk(self._lib.ef_matches_merge_topk(self._h, parts.data_ptr(), nparts, b, m, keys.data_ptr(),
                                                          None, N.EF_MEM_DEVICE))
        return keys

    def topk_stats(self):
        """(probes, probes whose first candidate list overflowed, probes resolved by the full
        fp64 sweep, candidate rows re-scored in fp64) of the most recent top-m search
        (ef_search_topk_stats); synchronises the stream."""
        out = (C.c_int64 * 4)()
        self._chk(self._lib.ef_search_topk_stats(self._h, out))
        return tuple(int(v) for v in out)

    def recognize(self, P, metric="l2", return_features=False):
        """Project probes P (uint8/float32 pixels) and return (idx, best[, feats])."""
        p = np.asarray(P)
        feats = np.empty((p.shape[0], self.model_k), dtype=np.float32) if return_features else None
        keys = self.recognize_keys(p, metric, feats=feats)
        idx, best = decode_keys(keys, metric)
        return (idx, best, feats) if return_features else (idx, best)

    # ------------------------------------------------------------------ model bank
    def bank_clear(self):
        """Drop every slot of the model bank and free its memory (ef_bank_clear)."""
        self._chk(self._lib.ef_bank_clear(self._h))
        self._bank_k = []
        self.bank_owner = None

    def bank_add(self, mean, W, G) -> int:
        """Append one (mean[d], W[d, k], gallery G[n, k]) triple to the model bank; returns its
        slot.  NumPy arrays or torch device tensors (all three alike); n may be 0."""
        if _is_dev(W):
            import torch
            m, mp = _dev(mean, torch.float32)
            w, wp = _dev(W, torch.float32)
            g, gp = _dev(G, torch.float32)
            flags = N.EF_MEM_DEVICE
        else:
            m, mp = _host(mean, np.float32)
            w, wp = _host(W, np.float32)
            g, gp = _host(G, np.float32)
            flags = 0
        if w.ndim != 2 or m.ndim != 1 or m.shape[0] != w.shape[0]:
            raise ValueError("mean must be (d,) and W (d, k)")
        if g.ndim != 2 or g.shape[1] != w.shape[1]:
            raise ValueError(f"G must be (n, {w.shape[1]}), got {tuple(g.shape)}")
        slot = C.c_int32(-1)
        self._chk(self._lib.ef_bank_add(self._h, mp, wp, int(w.shape[0]), int(w.shape[1]), gp if g.shape[0] else None,
                                        int(g.shape[0]), flags, C.byref(slot)))
        self._bank_k = self.bank_slot_widths() + [int(w.shape[1])]
        self.bank_owner = None
        return int(slot.value)

    def bank_info(self):
        """(slots, d, sum of k, sum of gallery rows) of the model bank; zeros when empty."""
        n, d, tk, tr = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.ef_bank_info(self._h, C.byref(n), C.byref(d), C.byref(tk), C.byref(tr)))
        return int(n.value), int(d.value), int(tk.value), int(tr.value)

    def bank_recognize_raw(self, P, metric="cosine", matches=False, features=False):
        """ef_bank_recognize on at most EF_BANK_MAX_PROBES probes: (keys[b, M] int64,
        records[b, M] or None, best_slot[b] int32, feats[b, sum k] or None) — NumPy for host
        pixels (N.MATCH_DTYPE records), torch tensors for device pixels ((b, M, 3) int64
        records; stream-ordered, not synchronised)."""
        mt = _metric(metric)
        M, d, tk, _ = self.bank_info()
        if M == 0:  # the library reports the state error
            self._chk(self._lib.ef_bank_recognize(self._h, None, N.EF_U8, 0, mt, None, None, None, None, 0))
        if _is_dev(P):
            import torch
            if P.dtype not in (torch.uint8, torch.float32):
                raise TypeError(f"probe pixels must be uint8 or float32, got {P.dtype}")
            if P.ndim != 2 or P.shape[1] != d:
                raise ValueError(f"P must be (b, {d}), got {tuple(P.shape)}")
            p, pp = _dev(P, P.dtype)
            b = p.shape[0]
            keys = torch.empty((b, M), dtype=torch.int64, device=p.device)
            rec = torch.empty((b, M, 3), dtype=torch.int64, device=p.device) if matches else None
            best = torch.empty(b, dtype=torch.int32, device=p.device)
            feats = torch.empty((b, tk), dtype=torch.float32, device=p.device) if features else None
            with self._torch_order(p, keys, rec, best, feats):
                self._chk(self._lib.ef_bank_recognize(
                    self._h, pp, N.EF_U8 if P.dtype == torch.uint8 else N.EF_F32, b, mt, keys.data_ptr(),
                    rec.data_ptr() if matches else None, best.data_ptr(), feats.data_ptr() if features else None,
                    N.EF_MEM_DEVICE))
            return keys, rec, best, feats
        p = np.asarray(P)
        dtype = N.EF_U8 if p.dtype == np.uint8 else N.EF_F32
        p, pp = _host(p, np.uint8 if dtype == N.EF_U8 else np.float32)
        if p.ndim != 2 or p.shape[1] != d:
            raise ValueError(f"P must be (b, {d}), got {p.shape}")
        b = p.shape[0]
        keys = np.empty((b, M), dtype=np.int64)
        rec = np.empty((b, M), dtype=N.MATCH_DTYPE) if matches else None
        best = np.empty(b, dtype=np.int32)
        feats = np.empty((b, tk), dtype=np.float32) if features else None
        self._chk(self._lib.ef_bank_recognize(self._h, pp, dtype, b, mt, keys.ctypes.data,
                                              rec.ctypes.data if matches else None, best.ctypes.data,
                                              feats.ctypes.data if features else None, 0))
        return keys, rec, best, feats

    def bank_recognize(self, P, metric="cosine", return_features=False):
        """Project the probes through every model of the bank and search every gallery:
        (idx[b, M] int64, score[b, M] float32, best_slot[b] int32[, feats]) as NumPy arrays —
        idx / score per slot as :meth:`search` gives them (idx -1, score NaN for an empty
        gallery), best_slot the reference's choice over models (-1: none), feats a list of M
        (b, k_m) arrays.  Batches over EF_BANK_MAX_PROBES probes run in chunks."""
        b = int(P.shape[0])
        chunk = N.EF_BANK_MAX_PROBES
        parts = [self.bank_recognize_raw(P[o:o + chunk], metric, features=return_features)
                 for o in range(0, max(b, 1), chunk)]
        if _is_dev(P):
            parts = [tuple(None if t is None else t.cpu().numpy() for t in part) for part in parts]
        keys = np.concatenate([part[0] for part in parts])
        best = np.concatenate([part[2] for part in parts])
        idx, score = decode_keys(keys.reshape(-1), metric)
        out = (idx.reshape(keys.shape), score.reshape(keys.shape), best)
        if not return_features:
            return out
        f = np.concatenate([part[3] for part in parts])
        ks = self.bank_slot_widths()
        offs = np.concatenate([[0], np.cumsum(ks)])
        return out + ([np.ascontiguousarray(f[:, offs[m]:offs[m + 1]]) for m in range(len(ks))],)

    def bank_set_reconstruction(self, slot, R, weight=None):
        """The way back of bank slot ``slot`` (ef_bank_recon_set): R (k, d) and an optional
        per-pixel weight (d,), as :meth:`set_reconstruction` takes them.  A failed call leaves the
        slot's previous state."""
        if _is_dev(R):
            import torch
            r, rp = _dev(R, torch.float32)
            w, wp = _dev(weight, torch.float32) if weight is not None else (None, None)
            flags = N.EF_MEM_DEVICE
        else:
            r, rp = _host(R, np.float32)
            w, wp = _host(weight, np.float32) if weight is not None else (None, None)
            flags = 0
        if r.ndim != 2:
            raise ValueError("R must be 2-D (k, d)")
        ks, d = self.bank_slot_widths(), self.bank_info()[1]
        if 0 <= int(slot) < len(ks) and tuple(r.shape) != (ks[int(slot)], d):  # (the library rejects a bad slot)
            raise ValueError(f"R must be ({ks[int(slot)]}, {d}), got {tuple(r.shape)}")
        if w is not None and tuple(w.shape) != (int(r.shape[1]),):
            raise ValueError("weight and R disagree on d")
        self._chk(self._lib.ef_bank_recon_set(self._h, int(slot), rp, wp, flags))

    def _bank_pixels(self, P, d):
        """(array or tensor, pointer, dtype code, b, on_device) of the probes of a bank call."""
        if _is_dev(P):
            import torch
            if P.dtype not in (torch.uint8, torch.float32):
                raise TypeError(f"probe pixels must be uint8 or float32, got {P.dtype}")
            if P.ndim != 2 or P.shape[1] != d:
                raise ValueError(f"P must be (b, {d}), got {tuple(P.shape)}")
            p, pp = _dev(P, P.dtype)
            return p, pp, (N.EF_U8 if P.dtype == torch.uint8 else N.EF_F32), int(p.shape[0]), True
        p = np.asarray(P)
        dtype = N.EF_U8 if p.dtype == np.uint8 else N.EF_F32
        p, pp = _host(p, np.uint8 if dtype == N.EF_U8 else np.float32)
        if p.ndim != 2 or p.shape[1] != d:
            raise ValueError(f"P must be (b, {d}), got {p.shape}")
        return p, pp, dtype, int(p.shape[0]), False

    def _split_feats(self, f):
        ks = self.bank_slot_widths()
        offs = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
        return [np.ascontiguousarray(f[:, offs[m]:offs[m + 1]]) for m in range(len(ks))]

    def bank_face_distance(self, P, return_energy=False, return_features=False):
        """Distance from face space of pixels P (b, d) against every slot of the bank
        (ef_bank_face_distance): eps2 (b, M) float32 and, when asked, the energy (b, M) and the
        features, in that order.  Host pixels give NumPy arrays (features as a list of M (b, k_m)
        arrays, the ones :meth:`bank_recognize` returns); device pixels give device tensors
        (features (b, sum k)), stream-ordered.  At most EF_BANK_MAX_PROBES probes per call."""
        M, d, tk, _ = self.bank_info()
        if M == 0:  # the library reports the state error
            self._chk(self._lib.ef_bank_face_distance(self._h, None, N.EF_U8, 0, None, None, None, 0))
        p, pp, dtype, b, dev = self._bank_pixels(P, d)
        if dev:
            import torch

            def alloc(shape):
                return torch.empty(shape, dtype=torch.float32, device=p.device)

            def ptr(a):
                return a.data_ptr() if a is not None else None
        else:
            def alloc(shape):
                return np.empty(shape, dtype=np.float32)

            def ptr(a):
                return a.ctypes.data if a is not None else None
        out = alloc((b, M))
        en = alloc((b, M)) if return_energy else None
        ft = alloc((b, tk)) if return_features else None
        ctx = self._torch_order(p, out, en, ft) if dev else contextlib.nullcontext()
        with ctx:
            self._chk(self._lib.ef_bank_face_distance(self._h, pp, dtype, b, ptr(out), ptr(en), ptr(ft),
                                                      N.EF_MEM_DEVICE if dev else 0))
        if ft is not None and not dev:
            ft = self._split_feats(ft)
        res = (out,) + ((en,) if return_energy else ()) + ((ft,) if return_features else ())
        return res[0] if len(res) == 1 else res

    def bank_recognize_gated_raw(self, P, gate, metric="cosine", relative=True, matches=False, features=False):
        """ef_bank_recognize_gated on at most EF_BANK_MAX_PROBES probes: (keys, records or None,
        best_slot, feats or None, dffs2[b, M], energy[b, M]) as :meth:`bank_recognize_raw` gives
        its four.  ``gate`` is (M,) float32: NumPy for host pixels, a device tensor (or an array,
        uploaded here) for device pixels."""
        mt = _metric(metric)
        M, d, tk, _ = self.bank_info()
        if M == 0:  # the library reports the state error
            one = np.zeros(1, np.float32)
            self._chk(self._lib.ef_bank_recognize_gated(self._h, None, N.EF_U8, 0, mt, one.ctypes.data, None, None, None,
                                                        None, None, None, 0))
        p, pp, dtype, b, dev = self._bank_pixels(P, d)
        flags = N.EF_BANK_GATE_RELATIVE if relative else 0
        g, gp = _gate_arg(gate, p.device if dev else None, M)
        if dev:
            import torch
            keys = torch.empty((b, M), dtype=torch.int64, device=p.device)
            rec = torch.empty((b, M, 3), dtype=torch.int64, device=p.device) if matches else None
            best = torch.empty(b, dtype=torch.int32, device=p.device)
            feats = torch.empty((b, tk), dtype=torch.float32, device=p.device) if features else None
            eps = torch.empty((b, M), dtype=torch.float32, device=p.device)
            en = torch.empty((b, M), dtype=torch.float32, device=p.device)
            with self._torch_order(p, g, keys, rec, best, feats, eps, en):
                self._chk(self._lib.ef_bank_recognize_gated(
                    self._h, pp, dtype, b, mt, gp, keys.data_ptr(), rec.data_ptr() if matches else None,
                    best.data_ptr(), eps.data_ptr(), en.data_ptr(), feats.data_ptr() if features else None,
                    flags | N.EF_MEM_DEVICE))
            return keys, rec, best, feats, eps, en
        keys = np.empty((b, M), dtype=np.int64)
        rec = np.empty((b, M), dtype=N.MATCH_DTYPE) if matches else None
        best = np.empty(b, dtype=np.int32)
        feats = np.empty((b, tk), dtype=np.float32) if features else None
        eps = np.empty((b, M), dtype=np.float32)
        en = np.empty((b, M), dtype=np.float32)
        self._chk(self._lib.ef_bank_recognize_gated(self._h, pp, dtype, b, mt, gp, keys.ctypes.data,
                                                    rec.ctypes.data if matches else None, best.ctypes.data,
                                                    eps.ctypes.data, en.ctypes.data,
                                                    feats.ctypes.data if features else None, flags))
        return keys, rec, best, feats, eps, en

    def bank_recognize_gated(self, P, gate, metric="cosine", relative=True, return_features=False):
        """:meth:`bank_recognize` with a face gate: (idx[b, M], score[b, M], best_slot[b][, feats],
        dffs2[b, M], energy[b, M]) as NumPy arrays.  idx, score and feats are bit-identical to
        :meth:`bank_recognize`'s; best_slot's walk over models skips slot m for probe p when
        ``dffs2[p, m] > gate[m]`` (``relative``: ``> gate[m] * energy[p, m]``, one float32 multiply)
        is true, so +inf or NaN gate nothing.  Batches over EF_BANK_MAX_PROBES run in chunks."""
        b = int(P.shape[0])
        chunk = N.EF_BANK_MAX_PROBES
        parts = [self.bank_recognize_gated_raw(P[o:o + chunk], gate, metric, relative, features=return_features)
                 for o in range(0, max(b, 1), chunk)]
        if _is_dev(P):
            parts = [tuple(None if t is None else t.cpu().numpy() for t in part) for part in parts]
        keys = np.concatenate([part[0] for part in parts])
        best = np.concatenate([part[2] for part in parts])
        eps = np.concatenate([part[4] for part in parts])
        en = np.concatenate([part[5] for part in parts])
        idx, score = decode_keys(keys.reshape(-1), metric)
        out = (idx.reshape(keys.shape), score.reshape(keys.shape), best)
        if return_features:
            out = out + (self._split_feats(np.concatenate([part[3] for part in parts])),)
        return out + (eps, en)

    def bank_slot_widths(self):
        """k of every slot added through this Engine since the last bank_clear."""
        return list(getattr(self, "_bank_k", []))

    # ---------------------------------------------------------------------- images
    PREPROCESS_CHUNK = 65535

    def preprocess(self, images, size=(64, 64), rgb=False, out=None):
        """Grey + INTER_LINEAR resize of a ragged batch (include/eigenface.h
        ef_preprocess): ``images`` is a list of uint8 arrays (h, w) or (h, w, 3|4)
        (BGR unless ``rgb``); ``size`` is cv2's (width, height).  Returns an
        (n, height*width) uint8 array (or fills device tensor ``out``)."""
        ow, oh = int(size[0]), int(size[1])
        n = len(images)
        if n == 0:
            return np.empty((0, oh * ow), np.uint8)
        if n > self.PREPROCESS_CHUNK:  # ef_preprocess takes at most 65535 images per call
            res = np.empty((n, oh * ow), np.uint8) if out is None else None
            for a in range(0, n, self.PREPROCESS_CHUNK):
                e = min(n, a + self.PREPROCESS_CHUNK)
                part = self.preprocess(images[a:e], size, rgb, None if out is None else out[a:e])
                if res is not None:
                    res[a:e] = part
            return out if out is not None else res
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in images]
        hs = np.array([a.shape[0] for a in arrs], np.int32)
        ws = np.array([a.shape[1] for a in arrs], np.int32)
        cs = np.array([1 if a.ndim == 2 else a.shape[2] for a in arrs], np.int32)
        sizes = np.array([a.size for a in arrs], np.int64)
        offs = np.zeros(n, np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        buf = np.concatenate([a.reshape(-1) for a in arrs])
        flags = N.EF_IMG_RGB if rgb else 0
        if out is not None:  # device output: stage the pixels on the device too
            import torch
            dbuf = torch.from_numpy(buf).to(out.device)
            with self._torch_order(out, dbuf):
                self._chk(self._lib.ef_preprocess(self._h, dbuf.data_ptr(), offs.ctypes.data, hs.ctypes.data,
                                                  ws.ctypes.data, cs.ctypes.data, n, oh, ow, out.data_ptr(),
                                                  flags | N.EF_MEM_DEVICE))
            return out
        res = np.empty((n, oh * ow), np.uint8)
        self._chk(self._lib.ef_preprocess(self._h, buf.ctypes.data, offs.ctypes.data, hs.ctypes.data,
                                          ws.ctypes.data, cs.ctypes.data, n, oh, ow, res.ctypes.data, flags))
        return res

    @staticmethod
    def _frame_view(frame):
        """(array or tensor, pointer, row stride in bytes, H, W, channels, on device) of a uint8
        frame (H, W) or (H, W, 1|3|4).  A view whose pixels are contiguous inside each row (a
        column slice of a wider frame) is passed as it is, with its row stride; anything else
        is copied."""
        dev = _is_dev(frame)
        if dev:
            import torch
            if frame.dtype != torch.uint8:
                raise TypeError(f"frame must be uint8, got {frame.dtype}")
            f = frame
            strides = tuple(int(v) for v in f.stride())
        else:
            f = np.asarray(frame)
            if f.dtype != np.uint8:
                raise TypeError(f"frame must be uint8, got {f.dtype}")
            strides = f.strides
        if f.ndim not in (2, 3) or 0 in f.shape:
            raise ValueError("frame must be (H, W) or (H, W, channels) and not empty")
        h, w = int(f.shape[0]), int(f.shape[1])
        ch = 1 if f.ndim == 2 else int(f.shape[2])
        inner = strides[1:] == ((1,) if f.ndim == 2 else (ch, 1))
        if not inner or strides[0] < w * ch:
            f = f.contiguous() if dev else np.ascontiguousarray(f)
            ld = w * ch
        else:
            ld = int(strides[0])
        return f, (f.data_ptr() if dev else f.ctypes.data), ld, h, w, ch, dev

    def preprocess_rois(self, frame, rects, size=(64, 64), rgb=False, out=None):
        """Grey + INTER_LINEAR resize of rectangles of one frame (include/eigenface.h
        ef_preprocess_rois): row i equals ``preprocess([frame[y:y+h, x:x+w]], size)[0]`` for
        ``rects[i] = (x, y, w, h)``, without the crops being copied out.  ``frame`` is a uint8
        array (H, W) or (H, W, 3|4) (BGR unless ``rgb``), or a device tensor; a row-strided
        view is read in place.  Host ``rects`` are validated (a bad one raises).  With a
        device frame, ``rects`` may be a device int32 tensor (n, 4): the call is then
        stream-ordered with no host wait, and the kernel clips each rectangle to the frame (a
        zero row for an empty one or a negative origin).  Returns (n, height*width) uint8:
        NumPy for a host frame, a device tensor (``out`` when given) for a device frame."""
        ow, oh = int(size[0]), int(size[1])
        f, fp, ld, h, w, ch, dev = self._frame_view(frame)
        flags = N.EF_IMG_RGB if rgb else 0
        if _is_dev(rects):
            import torch
            if not dev:
                raise TypeError("device rectangles need a device frame")
            r, rp = _dev(rects, torch.int32)
            flags |= N.EF_ROI_RECTS_DEVICE
        else:
            r, rp = _host(rects, np.int32)
        if r.shape[0] and (r.ndim != 2 or r.shape[1] != 4):
            raise ValueError("rects must be (n, 4): x, y, w, h")
        n = int(r.shape[0])
        if not dev:
            res = np.empty((n, oh * ow), np.uint8)
            self._chk(self._lib.ef_preprocess_rois(self._h, fp, ld, h, w, ch, rp, n, oh, ow, res.ctypes.data, flags))
            return res
        import torch
        if out is None:
            out = torch.empty((n, oh * ow), dtype=torch.uint8, device=f.device)
        self._dev_out(out, (n, oh * ow), torch.uint8, "out")
        with self._torch_order(f, out, r if _is_dev(r) else None):
            self._chk(self._lib.ef_preprocess_rois(self._h, fp, ld, h, w, ch, rp, n, oh, ow, out.data_ptr(),
                                                   flags | N.EF_MEM_DEVICE))
        return out

    # ----------------------------------------------------------------- JPEG decode
    def decode_jpegs(self, blobs, mode="bgr"):
        """GPU decode of a batch of JPEG files (include/eigenface.h ef_jpeg_decode):
        ``blobs`` are the files' bytes; ``mode`` "bgr" (cv2.imread IMREAD_COLOR) or "gray"
        (IMREAD_GRAYSCALE).  Returns a list of uint8 arrays, None where the GPU decoder
        does not take the file (progressive, CMYK, ...; ``status`` says why)."""
        m = _jpeg_mode(mode)
        n = len(blobs)
        if n == 0:
            return []
        packed = _pack_blobs(blobs)
        data, offs, sizes, _keep = packed
        h, w, _, st = jpeg_info(blobs, _packed=packed)
        ch = 1 if m == N.EF_JPEG_GRAY else 3
        px = np.where(st == 0, h.astype(np.int64) * w * ch, 0)
        ooff = np.zeros(n, np.int64)
        ooff[1:] = np.cumsum(px)[:-1]
        out = np.empty(max(1, int(px.sum())), np.uint8)
        self._chk(self._lib.ef_jpeg_decode(self._h, data, offs.ctypes.data, sizes.ctypes.data, n, m,
                                           out.ctypes.data, ooff.ctypes.data, st.ctypes.data, 0))
        res = []
        for i in range(n):
            if st[i] != 0:
                res.append(None)
                continue
            a = out[ooff[i]:ooff[i] + px[i]]
            res.append(a.reshape(h[i], w[i]) if ch == 1 else a.reshape(h[i], w[i], 3))
        return res

    def ingest_jpegs(self, blobs, size=(64, 64), mode="bgr", out=None):
        """Fused GPU decode + grey + INTER_LINEAR resize of JPEG files
        (ef_jpeg_ingest): (rows uint8 (n, h*w) — or device tensor ``out`` filled —,
        status int32 (n,)).  Rows of files with status != 0 are zero.  With ``out`` the
        call returns once the decode is queued on the engine's stream (status is final);
        torch's current stream is ordered after it (no host wait), so torch work on ``out``
        queued afterwards sees the decoded rows, and back-to-back calls overlap one batch's
        host staging with the previous batch's decode."""
        m = _jpeg_mode(mode)
        ow, oh = int(size[0]), int(size[1])
        n = len(blobs)
        st = np.zeros(n, np.int32)
        if n == 0:
            return np.empty((0, oh * ow), np.uint8), st
        data, offs, sizes, _keep = _pack_blobs(blobs)
        if out is not None:
            import torch
            o, op = _dev(out, torch.uint8)
            self._dev_out(o, (n, oh * ow), torch.uint8, "out")
            with self._torch_order(o):
                self._chk(self._lib.ef_jpeg_ingest(self._h, data, offs.ctypes.data, sizes.ctypes.data, n, m,
                                                   oh, ow, op, st.ctypes.data, N.EF_MEM_DEVICE))
            return out, st
        rows = np.empty((n, oh * ow), np.uint8)
        self._chk(self._lib.ef_jpeg_ingest(self._h, data, offs.ctypes.data, sizes.ctypes.data, n, m,
                                           oh, ow, rows.ctypes.data, st.ctypes.data, 0))
        return rows, st

    def tm_prepare(self, templates, problems, frame_shape):
        """Resident template-localiser operands (ef_tm_prepare).  ``templates``: list of
        grey uint8 (h, w) arrays; ``problems``: list of (template index, height, width)
        scaled sizes; ``frame_shape``: (H, W)."""
        arrs = [np.ascontiguousarray(t, dtype=np.uint8) for t in templates]
        nt = len(arrs)
        th = np.array([a.shape[0] for a in arrs], np.int32)
        tw = np.array([a.shape[1] for a in arrs], np.int32)
        sizes = np.array([a.size for a in arrs], np.int64)
        offs = np.zeros(nt, np.int64)
        if nt > 1:
            offs[1:] = np.cumsum(sizes)[:-1]
        buf = np.concatenate([a.reshape(-1) for a in arrs]) if nt else np.zeros(1, np.uint8)
        pr = np.asarray(problems, dtype=np.int64).reshape(-1, 3)
        pt, ph, pw = (np.ascontiguousarray(pr[:, i], dtype=np.int32) for i in range(3))
        H, W = (int(v) for v in frame_shape)
        self._scan = self.scan_owner = None  # a new localiser drops the frame scan's plan
        self._chk(self._lib.ef_tm_prepare(self._h, buf.ctypes.data, offs.ctypes.data, th.ctypes.data,
                                          tw.ctypes.data, nt, pt.ctypes.data, ph.ctypes.data, pw.ctypes.data,
                                          len(pr), H, W, 0))
        self._tm = (len(pr), H, W, pr.copy())

    def tm_match(self, frame, maps=False):
        """Run the prepared problems on one grey frame: (best float32[P], x int32[P],
        y int32[P]) and, with ``maps``, the list of TM_CCOEFF_NORMED result maps."""
        if getattr(self, "_tm", None) is None:
            raise RuntimeError("call tm_prepare first")
        npb, H, W, _ = self._tm
        f = np.ascontiguousarray(frame, dtype=np.uint8)
        if f.shape != (H, W):
            raise ValueError(f"frame must be {(H, W)}, got {f.shape}")
        best = np.empty(npb, np.float32)
        xs = np.empty(npb, np.int32)
        ys = np.empty(npb, np.int32)
        mp = None
        if maps:
            n = C.c_int32(0)
            tot = C.c_int64(0)
            hr = np.empty(max(npb, 1), np.int32)
            wr = np.empty(max(npb, 1), np.int32)
            self._chk(self._lib.ef_tm_info(self._h, C.byref(n), C.byref(tot), hr.ctypes.data, wr.ctypes.data))
            flat = np.empty(tot.value, np.float32)
            mp = flat
        self._chk(self._lib.ef_tm_match(self._h, f.ctypes.data, W, best.ctypes.data, xs.ctypes.data,
                                        ys.ctypes.data, mp.ctypes.data if mp is not None else None, 0))
        if not maps:
            return best, xs, ys
        out, o = [], 0
        for p in range(npb):
            m = int(hr[p]) * int(wr[p])
            out.append(flat[o:o + m].reshape(int(hr[p]), int(wr[p])))
            o += m
        return best, xs, ys, out

    # ----------------------------------------------------------------- frame scan
    def scan_prepare(self, prob_group, n_groups, face_size=(64, 64), threshold=0.6):
        """The frame scan's plan over the prepared localiser (ef_scan_prepare): problem p
        belongs to group (person) ``prob_group[p]``; faces are resized to cv2's ``face_size``
        (width, height).  A later tm_prepare drops the plan."""
        if getattr(self, "_tm", None) is None:  # the library reports the state error
            self._chk(self._lib.ef_scan_prepare(self._h, None, int(n_groups), 1, 1, float(threshold)))
        g, gp = _host(prob_group, np.int32)
        if g.ndim != 1 or g.shape[0] != self._tm[0]:
            raise ValueError(f"prob_group must have one group per problem ({self._tm[0]})")
        fw, fh = int(face_size[0]), int(face_size[1])
        self._chk(self._lib.ef_scan_prepare(self._h, gp if g.shape[0] else None, int(n_groups), fh, fw,
                                            float(threshold)))
        self._scan = (int(n_groups), fh, fw)

    def scan_frame(self, frame, metric="cosine", rgb=False):
        """One frame through grey, localiser, selection, ROI rows and the model bank
        (ef_scan_frame): (dets, keys[G, M] int64, best_slot[G] int32, rows[G, h*w] uint8) for
        the plan's G groups and the bank's M slots.  ``frame`` is (H, W) grey or (H, W, 3|4)
        BGR(A) (RGB(A) with ``rgb``) of the prepared frame size.  A host frame gives NumPy
        arrays, dets as records of N.SCAN_DET_DTYPE, after one upload, one download and one
        synchronisation; a device tensor gives device tensors, dets as (G, 8) int32 in the
        fields' order (confidence as float32 bits), stream-ordered with no host wait."""
        mt = _metric(metric)
        if getattr(self, "_tm", None) is None or getattr(self, "_scan", None) is None:
            # the library reports the state error
            self._chk(self._lib.ef_scan_frame(self._h, None, 0, 1, mt, None, None, None, None, 0))
            raise RuntimeError("call scan_prepare first")
        return self._scan_frame(frame, mt, False, None, False, rgb)

    def _scan_frame(self, frame, mt, gated, gate, relative, rgb):
        """scan_frame (ef_scan_frame) and, ``gated``, scan_frame_gated (ef_scan_frame_gated)."""
        (G, fh, fw), H, W = self._scan, self._tm[1], self._tm[2]
        f, fp, ld, h, w, ch, dev = self._frame_view(frame)
        if (h, w) != (H, W):
            raise ValueError(f"frame must be {(H, W)}, got {(h, w)}")
        M = self.bank_info()[0]
        device = f.device if dev else None
        flags = ((N.EF_IMG_RGB if rgb else 0) | (N.EF_BANK_GATE_RELATIVE if gated and relative else 0) |
                 (N.EF_MEM_DEVICE if dev else 0))
        g, gp = _gate_arg(gate, device, M) if gated else (None, None)
        dets = _empty((G, 8), np.int32, device) if dev else np.empty(G, dtype=N.SCAN_DET_DTYPE)
        out = _frame_outputs(G, M, fh * fw, gated, device)
        args = [_ptr(a) for a in [dets] + out] + [flags]
        with self._torch_order(f, g, dets, *out) if dev else contextlib.nullcontext():
            if gated:
                self._chk(self._lib.ef_scan_frame_gated(self._h, fp, ld, ch, mt, gp, *args))
            else:
                self._chk(self._lib.ef_scan_frame(self._h, fp, ld, ch, mt, *args))
        return (dets, *out)

    def scan_frame_gated(self, frame, gate, metric="cosine", relative=True, rgb=False):
        """:meth:`scan_frame` whose recognition step is :meth:`bank_recognize_gated`
        (ef_scan_frame_gated): (dets, keys, best_slot, rows, dffs2[G, M], energy[G, M]).  dets, keys
        and rows are :meth:`scan_frame`'s, bit for bit; best_slot skips the slots ``gate`` (M,)
        rejects."""
        mt = _metric(metric)
        if getattr(self, "_tm", None) is None or getattr(self, "_scan", None) is None:
            one = np.zeros(1, np.float32)  # the library reports the state error
            self._chk(self._lib.ef_scan_frame_gated(self._h, None, 0, 1, mt, one.ctypes.data, None, None, None, None,
                                                    None, None, 0))
            raise RuntimeError("call scan_prepare first")
        return self._scan_frame(frame, mt, True, gate, relative, rgb)

    # ------------------------------------------------------ Haar route in one call
    def haar_group(self, rects, min_neighbors=3, max_rects=None):
        """cv2.groupRectangles(rects, min_neighbors, 0.2) on the GPU (ef_haar_group): the grouped
        rectangles of ``rects`` (n, 4) int32 ``x, y, w, h`` in OpenCV's order, value for value what
        the detector's host grouping returns.  ``min_neighbors`` must be at least 1.  A host array
        gives a NumPy (m, 4) array; a device tensor gives ``(out, n_rects)`` device tensors, ``out``
        (max_rects, 4) zero behind the first ``n_rects`` rows, stream-ordered with no host wait.
        More than N.EF_HAAR_GROUP_MAX rectangles raise (EF_HAAR_SCAN_OVERFLOW)."""
        if _is_dev(rects):
            import torch
            r, rp = _dev(rects, torch.int32)
        else:
            r, rp = _host(rects, np.int32)
        n = int(r.shape[0])
        if n and (r.ndim != 2 or r.shape[1] != 4):
            raise ValueError("rects must be (n, 4): x, y, w, h")
        cap = n if max_rects is None else int(max_rects)
        if _is_dev(rects):
            out = torch.empty((cap, 4), dtype=torch.int32, device=r.device)
            cnt = torch.empty(1, dtype=torch.int32, device=r.device)
            with self._torch_order(r, out, cnt):
                self._chk(self._lib.ef_haar_group(self._h, rp if n else None, n, int(min_neighbors),
                                                  out.data_ptr() if cap else None, cap, cnt.data_ptr(),
                                                  N.EF_MEM_DEVICE))
            return out, cnt
        out = np.zeros((cap, 4), np.int32)
        cnt = C.c_int32(0)
        self._chk(self._lib.ef_haar_group(self._h, rp if n else None, n, int(min_neighbors),
                                          out.ctypes.data if cap else None, cap, C.byref(cnt), 0))
        return out[:min(cnt.value, cap)].copy()

    def haar_scan_prepare(self, frame_shape, scale_factor=1.1, min_neighbors=5, min_size=(30, 30), max_size=(),
                          face_size=(64, 64), max_faces=8, max_candidates=4096):
        """The Haar frame scan's plan (ef_haar_scan_prepare) for frames of ``frame_shape`` (H, W)
        over the loaded cascade: the detectMultiScale parameters, cv2's ``face_size`` (width,
        height) of the recognised crops, the ``max_faces`` rectangles a frame is recognised for and
        the ``max_candidates`` the grouping kernels take.  A new cascade drops the plan."""
        H, W = int(frame_shape[0]), int(frame_shape[1])
        mn = tuple(min_size) if min_size else (0, 0)
        mx = tuple(max_size) if max_size else (0, 0)
        fw, fh = int(face_size[0]), int(face_size[1])
        self._haar_scan = None
        self._chk(self._lib.ef_haar_scan_prepare(self._h, H, W, float(scale_factor), int(min_neighbors), int(mn[0]),
                                                 int(mn[1]), int(mx[0]), int(mx[1]), fh, fw, int(max_faces),
                                                 int(max_candidates)))
        self._haar_scan = (H, W, fh, fw, int(max_faces))

    def haar_scan_info(self):
        """(pyramid layers, visitable-window bound, max_faces, max_candidates) of the plan."""
        nl, vis, mf, mc = C.c_int32(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.ef_haar_scan_info(self._h, C.byref(nl), C.byref(vis), C.byref(mf), C.byref(mc)))
        return int(nl.value), int(vis.value), int(mf.value), int(mc.value)

    def haar_scan_frame(self, frame, metric="cosine", gate=None, relative=True, rgb=False):
        """One frame through grey, the Haar detector, the rectangle grouping, the ROI rows and
        the model bank (ef_haar_scan_frame): (head, rects[F, 4] int32, keys[F, M] int64,
        best_slot[F] int32, rows[F, h*w] uint8) for the plan's F = max_faces and the bank's M
        slots, and with ``gate`` (M,) also (dffs2[F, M], energy[F, M]) as
        :meth:`bank_recognize_gated` gives them.  ``head`` holds status, n_candidates, n_rects and
        n_faces = min(n_rects, F); rows and rectangles behind n_faces are zero.  A status with
        N.EF_HAAR_SCAN_OVERFLOW means nothing was grouped: redo the frame with the separate calls.
        A host frame gives NumPy arrays (head a record of N.HAAR_SCAN_HEAD_DTYPE) after one
        upload, one download and one synchronisation; a device tensor gives device tensors (head
        as (4,) int32), stream-ordered with no host wait."""
        mt = _metric(metric)
        plan = getattr(self, "_haar_scan", None)
        if plan is None:  # the library reports the state error
            hd = np.zeros(4, np.int32)
            self._chk(self._lib.ef_haar_scan_frame(self._h, hd.ctypes.data, 1, 1, mt, None, hd.ctypes.data,
                                                   hd.ctypes.data, hd.ctypes.data, None, None, None, None, 0))
            raise RuntimeError("call haar_scan_prepare first")
        H, W, fh, fw, F = plan
        f, fp, ld, h, w, ch, dev = self._frame_view(frame)
        if (h, w) != (H, W):
            raise ValueError(f"frame must be {(H, W)}, got {(h, w)}")
        M = self.bank_info()[0]
        device = f.device if dev else None
        gated = gate is not None
        flags = ((N.EF_IMG_RGB if rgb else 0) | (N.EF_BANK_GATE_RELATIVE if gated and relative else 0) |
                 (N.EF_MEM_DEVICE if dev else 0))
        g, gp = _gate_arg(gate, device, M) if gated else (None, None)
        head = _empty(4, np.int32, device) if dev else np.zeros(1, dtype=N.HAAR_SCAN_HEAD_DTYPE)
        rects = _empty((F, 4), np.int32, device)
        out = _frame_outputs(F, M, fh * fw, gated, device)
        args = [_ptr(a) for a in [head, rects] + out] + [None] * (5 - len(out)) + [flags]
        with self._torch_order(f, g, head, rects, *out) if dev else contextlib.nullcontext():
            self._chk(self._lib.ef_haar_scan_frame(self._h, fp, ld, ch, mt, gp, *args))
        return (head if dev else head[0], rects, *out)

    # --------------------------------------------------------------------- timing
    def timing(self, on=True):
        self._chk(self._lib.ef_timing_enable(self._h, 1 if on else 0))

    def timing_reset(self):
        self._chk(self._lib.ef_timing_reset(self._h))

    def timing_get(self, kernel="search"):
        kid = {"search": N.EF_KERNEL_SEARCH, "project": N.EF_KERNEL_PROJECT, "tmatch": N.EF_KERNEL_TMATCH,
               "ingest": N.EF_KERNEL_INGEST, "haar": N.EF_KERNEL_HAAR, "jpeg": N.EF_KERNEL_JPEG,
               "syrk": N.EF_KERNEL_SYRK, "jpeg_host": N.EF_KERNEL_JPEG_HOST, "scan": N.EF_KERNEL_SCAN,
               "recon": N.EF_KERNEL_RECON, "recon_reduce": N.EF_KERNEL_RECON_REDUCE,
               "haar_scan": N.EF_KERNEL_HAAR_SCAN, "cluster": N.EF_KERNEL_CLUSTER, "range": N.EF_KERNEL_RANGE,
               "rank": N.EF_KERNEL_RANK}[kernel]
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._chk(self._lib.ef_timing_get(self._h, kid, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)


def bank_recon_schedule(b, d, n_models):
    """ef_bank_recon_schedule (host only): the grouped residual's plan for b probes of d pixels
    against n_models slots, as a dict of nsplit, tiles_per_split, n_workgroups, scratch_bytes."""
    ns, tps, nwg, sb = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
    rc = N.lib().ef_bank_recon_schedule(int(b), int(d), int(n_models), C.byref(ns), C.byref(tps), C.byref(nwg),
                                        C.byref(sb))
    if rc != N.EF_OK:
        raise N.EigenfaceError(rc, "ef_bank_recon_schedule: bad arguments")
    return {"nsplit": int(ns.value), "tiles_per_split": int(tps.value), "n_workgroups": int(nwg.value),
            "scratch_bytes": int(sb.value)}


def decode_keys(keys, metric="l2"):
    """(idx int64, best float32) from packed keys; EF_KEY_NONE -> (-1, nan)."""
    k = np.ascontiguousarray(keys, dtype=np.int64)
    b = k.shape[0]
    idx = np.empty(b, dtype=np.int64)
    best = np.empty(b, dtype=np.float32)
    N.lib().ef_keys_decode(k.ctypes.data, b, _metric(metric), best.ctypes.data, idx.ctypes.data)
    return idx, best


def _decode_topk(keys, metric):
    """(idx (b, m), best (b, m)) of top-m keys (device tensor or host array)."""
    if _is_dev(keys):
        keys = keys.cpu().numpy()
    idx, best = decode_keys(np.ascontiguousarray(keys).reshape(-1), metric)
    return idx.reshape(keys.shape), best.reshape(keys.shape)


def merge_topk_host(parts, b, m):
    """Host merge (ef_matches_merge_topk without a context; no GPU needed) of nparts * b * m
    top-m records, part-major: an array of N.MATCH_DTYPE (any shape) or its int64 view
    (.., 3) -> int64 keys (b, m)."""
    b, m = int(b), int(m)
    p = np.ascontiguousarray(parts)
    if p.dtype != np.dtype(N.MATCH_DTYPE):
        p = np.ascontiguousarray(p, dtype=np.int64)
        if p.ndim < 2 or p.shape[-1] != 3:
            raise ValueError(f"parts must be int64 records (.., 3) or MATCH_DTYPE records, got {p.shape}")
        p = p.reshape(-1, 3).view(N.MATCH_DTYPE)
    p = p.reshape(-1)
    if not 1 <= m <= N.EF_TOPK_MAX:
        raise ValueError(f"m must be 1 .. {N.EF_TOPK_MAX}, got {m}")
    if b < 0 or (b and p.shape[0] % (b * m)) or (b == 0 and p.shape[0]):
        raise ValueError(f"{p.shape[0]} records is not a multiple of b * m = {b * m}")
    nparts = p.shape[0] // (b * m) if b else 0
    keys = np.empty((b, m), dtype=np.int64)
    if b:
        rc = N.lib().ef_matches_merge_topk(None, p.ctypes.data, nparts, b, m, keys.ctypes.data, None, 0)
        if rc != N.EF_OK:
            raise N.EigenfaceError(rc, "ef_matches_merge_topk failed")
    return keys


def merge_matches_host(parts, b):
    """Host merge (ef_matches_merge without a context; no GPU needed): ``parts`` is an
    array of N.MATCH_DTYPE (nparts*b, part-major) or its (nparts*b, 3) int64 view."""
    p = np.ascontiguousarray(parts)
    if p.dtype != np.dtype(N.MATCH_DTYPE):
        p = np.ascontiguousarray(p, dtype=np.int64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"parts must be (nparts*b, 3) int64 or MATCH_DTYPE records, got {p.shape}")
        p = p.view(N.MATCH_DTYPE).reshape(-1)
    b = int(b)
    if b < 0 or (b and p.shape[0] % b) or (b == 0 and p.shape[0]):
        raise ValueError(f"{p.shape[0]} records is not a multiple of b = {b}")
    nparts = p.shape[0] // b if b else 0
    keys = np.empty(b, dtype=np.int64)
    if b:
        rc = N.lib().ef_matches_merge(None, p.ctypes.data, nparts, b, keys.ctypes.data, None, 0)
        if rc != N.EF_OK:
            raise N.EigenfaceError(rc, "ef_matches_merge failed")
    return keys


def _jpeg_mode(mode):
    try:
        return {"bgr": N.EF_JPEG_BGR, "color": N.EF_JPEG_BGR, "gray": N.EF_JPEG_GRAY, "grey": N.EF_JPEG_GRAY}[mode]
    except KeyError:
        raise ValueError(f"unknown JPEG output mode {mode!r} (bgr | gray)") from None


def _bytes_data_offset():
    """Offset of a bytes object's payload from id(): CPython's PyBytesObject layout,
    verified once (0 disables the fast path)."""
    probe = b"eigenface-probe"
    off = sys.getsizeof(b"") - 1
    try:
        if C.string_at(id(probe) + off, len(probe)) == probe:
            return off
    except Exception:  # pragma: no cover - non-CPython
        pass
    return 0


_BYTES_OFF = None


def _pack_blobs(blobs):
    """Address the files in place (no concatenation): (base pointer, int64 offsets from it,
    int64 sizes, keep-alive list).  The C ABI reads file i at base + offsets[i]."""
    global _BYTES_OFF
    if _BYTES_OFF is None:
        _BYTES_OFF = _bytes_data_offset()
    n = len(blobs)
    sizes = np.fromiter(map(len, blobs), np.int64, n)
    if _BYTES_OFF and set(map(type, blobs)) == {bytes}:  # payload address = id + header
        addrs = np.fromiter(map(id, blobs), np.int64, n) + _BYTES_OFF
        keep = blobs
    else:
        keep = [np.frombuffer(b, np.uint8) if len(b) else np.zeros(1, np.uint8) for b in blobs]
        addrs = np.fromiter((v.ctypes.data for v in keep), np.int64, n)
    base = int(addrs.min()) if n else 0
    return base, addrs - base, sizes, keep


def jpeg_info(blobs, _packed=None):
    """Header parse on the host (ef_jpeg_info, no GPU): (height, width, components,
    status) int32 arrays; status 0 = the GPU decoder takes the file."""
    data, offs, sizes, _keep = _packed if _packed is not None else _pack_blobs(blobs)
    n = len(sizes)
    h, w, c, st = (np.zeros(n, np.int32) for _ in range(4))
    if n:
        rc = N.lib().ef_jpeg_info(data, offs.ctypes.data, sizes.ctypes.data, n, h.ctypes.data,
                                  w.ctypes.data, c.ctypes.data, st.ctypes.data)
        if rc != N.EF_OK:
            raise N.EigenfaceError(rc, "ef_jpeg_info failed")
    return h, w, c, st


def device_count() -> int:
    n = C.c_int(0)
    N.lib().ef_device_count(C.byref(n))
    return int(n.value)
