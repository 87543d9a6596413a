"""Gallery clustering: identity labels for unlabelled faces.

The reference project gets one identity per crop by hand: ``train-v5.py`` takes the name of the
directory a person sorted the crops into, the older trainers ask for a name at the prompt.
``cluster_gallery`` / ``cluster_faces`` group the rows on the GPU instead (``ef_gallery_cluster``: a
self-join of the resident gallery that links every pair within a threshold, every edge decided as
in fp64, and returns the connected components).

The threshold is the one ``equal_error_threshold`` / ``pair_equal_error`` give on a labelled
sample: a squared L2 distance (linked at or below it) or a cosine similarity (linked at or above
it).  The labels that come out are what ``Engine.set_gallery_labels``, ``score_census`` and
``Fisherfaces`` take; ``representatives`` (the lowest row of every cluster) is the keep-list for
de-duplication.

``pair_confusion`` and ``pairwise_scores`` compare a clustering with known identities from integer
pair counts (host code).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class ClusterResult:
    """Outcome of ``cluster_gallery``.  ``labels`` int32 (n,): clusters are numbered by their lowest
    member row, noise rows (only with ``min_samples`` > 1) are -1.  ``sizes`` int64 (n_clusters,)
    and ``representatives`` int64 (n_clusters,): the member count and the lowest row of each
    cluster.  ``degree`` int32 (n,) or None: rows linked to each row.  ``info`` int64 (4,):
    clusters, noise rows, linked unordered pairs, pairs settled in fp64."""

    labels: np.ndarray
    n_clusters: int
    sizes: np.ndarray
    representatives: np.ndarray
    degree: np.ndarray | None
    info: np.ndarray

    @property
    def n_noise(self):
        return int(self.info[1])

    @property
    def n_links(self):
        return int(self.info[2])


def cluster_gallery(eng, threshold, metric="l2", min_samples=1, degree=False):
    """Cluster the rows resident in ``eng`` (``Engine.set_gallery``) and return a ClusterResult."""
    labels, deg, info = eng.cluster_gallery(threshold, metric, min_samples, degree)
    nc = int(info[0])
    kept = labels >= 0
    sizes = np.bincount(labels[kept], minlength=nc).astype(np.int64)
    reps = np.full(nc, -1, np.int64)
    rows = np.flatnonzero(kept)
    # the first row of each label in row order is its lowest member
    lab, first = np.unique(labels[kept], return_index=True)
    reps[lab] = rows[first]
    return ClusterResult(labels, nc, sizes, reps, deg, info)


def cluster_faces(model_or_engine, faces, threshold, metric="l2", min_samples=1, degree=False):
    """Project ``faces`` (n, d) pixels, load the features as the gallery and cluster them.
    ``model_or_engine``: a fitted ``EigenfacePCA`` / ``Fisherfaces`` (anything with ``transform``;
    the features are clustered on an engine of their own, so the model's resident gallery stays),
    or an ``Engine`` holding a model (its gallery is replaced by the features)."""
    from .engine import Engine
    if isinstance(model_or_engine, Engine):
        eng = model_or_engine
        feats = np.ascontiguousarray(eng.project(np.asarray(faces)), dtype=np.float32)
    else:
        from .pca import get_engine
        feats = np.ascontiguousarray(model_or_engine.transform(faces), dtype=np.float32)
        eng = get_engine(getattr(model_or_engine, "device", 0), pool="cluster")
    eng.set_gallery(feats)
    return cluster_gallery(eng, threshold, metric, min_samples, degree)


def cluster_schedule(n, kp):
    """ef_cluster_schedule (host only): the link pass's work items for n rows of padded length kp,
    an int64 array (n_items, 3) of {first row tile, end row tile, probe tile}."""
    import ctypes as C
    lib = N.lib()
    cnt = C.c_int32(0)
    rc = lib.ef_cluster_schedule(int(n), int(kp), None, 0, C.byref(cnt))
    if rc != N.EF_OK:
        raise N.EigenfaceError(rc, "ef_cluster_schedule: bad arguments")
    items = np.zeros((cnt.value, 3), np.int64)
    if cnt.value:
        rc = lib.ef_cluster_schedule(int(n), int(kp), items.ctypes.data, cnt.value, C.byref(cnt))
        if rc != N.EF_OK:
            raise N.EigenfaceError(rc, "ef_cluster_schedule: bad arguments")
    return items


def _pairs(c):
    c = np.asarray(c, dtype=np.int64)
    return c * (c - 1) // 2


def pair_confusion(true, pred):
    """Pair counts of a clustering ``pred`` against identities ``true`` (any hashable values; -1 in
    ``pred`` marks noise, and every noise row counts as a cluster of its own), from the contingency
    table in integers: ``(tp, fp, fn, tn)`` of unordered row pairs, with positive = "same cluster"
    and true = "same identity".  tp + fp + fn + tn = n (n - 1) / 2."""
    t = np.asarray(true).ravel()
    p = np.asarray(pred).ravel()
    if t.shape != p.shape:
        raise ValueError(f"true and pred must have the same length, got {t.shape} and {p.shape}")
    n = t.shape[0]
    _, ti = np.unique(t, return_inverse=True)
    p = p.astype(np.int64, copy=True) if p.dtype.kind in "iu" else np.unique(p, return_inverse=True)[1].astype(np.int64)
    noise = p < 0
    if noise.any():  # singletons above every other label
        p[noise] = (p.max(initial=-1) + 1) + np.arange(int(noise.sum()))
    _, pi = np.unique(p, return_inverse=True)
    nt, npred = int(ti.max(initial=-1)) + 1, int(pi.max(initial=-1)) + 1
    cells = np.unique(ti.astype(np.int64) * max(npred, 1) + pi, return_counts=True)[1]
    same_both = int(_pairs(cells).sum())
    same_true = int(_pairs(np.bincount(ti, minlength=nt)).sum())
    same_pred = int(_pairs(np.bincount(pi, minlength=npred)).sum())
    total = n * (n - 1) // 2
    tp = same_both
    fp = same_pred - same_both
    fn = same_true - same_both
    return tp, fp, fn, total - tp - fp - fn


def pairwise_scores(true, pred):
    """``{"precision", "recall", "f1"}`` of the row pairs (pair_confusion); a ratio with an empty
    denominator is 1.0 (nothing claimed, or nothing to find)."""
    tp, fp, fn, _ = pair_confusion(true, pred)
    prec = tp / (tp + fp) if tp + fp else 1.0
    rec = tp / (tp + fn) if tp + fn else 1.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec else 0.0
    return {"precision": prec, "recall": rec, "f1": f1}
