"""Leave-one-out evaluation of a labelled gallery: rank-1 accuracy and the open-set error
rates a cosine / L2 acceptance threshold gives on the user's own data.

The GPU part is ``leave_one_out``: every gallery row is a probe, its own row is left out, and
the labelled search (``Engine.search_labelled_keys``) returns the nearest row of the same
identity (the genuine match) and the nearest row of any other identity (the impostor), each
with the guarantee of the plain search.  Everything else is host arithmetic on those two
arrays of packed keys, so it is usable (and tested) without a GPU.

Definitions, for a probe whose identity is enrolled (it has a genuine row):
  accept(score, t)   score >= t for cosine (similarity), score <= t for L2 (squared distance)
  rank-1 correct     genuine_key < impostor_key: a packed key orders by score, then by row, and
                     EF_KEY_NONE is the largest key, i.e. what a search of the whole gallery
                     without the probe's own row would return first
  FNIR(t)            share of the probes with a genuine row that are NOT (rank-1 correct and
                     accepted at t): an enrolled person missed
  FPIR(t)            share of the probes with an impostor row whose impostor is accepted at t:
                     the probe's person treated as not enrolled, somebody else answers
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as N
from .engine import decode_keys

REFERENCE_THRESHOLDS = (0.7, 0.8)  # scan-template-v4.py:270 / :289, :400 (cosine similarity)


@dataclass
class OpenSetRates:
    thresholds: np.ndarray  # candidates, ascending
    fnir: np.ndarray        # NaN when no probe has a genuine row
    fpir: np.ndarray        # NaN when no probe has an impostor row
    rank1: float            # rank-1 accuracy over the probes with a genuine row (NaN: none)


def _accept(score, t, metric):
    return score >= t if metric == "cosine" else score <= t


def _metric_name(metric):
    m = str(metric).lower()
    if m not in ("cosine", "l2"):
        raise ValueError(f"metric must be 'cosine' or 'l2', got {metric!r}")
    return m


def _keys(genuine_key, impostor_key):
    g = np.ascontiguousarray(genuine_key, dtype=np.int64)
    i = np.ascontiguousarray(impostor_key, dtype=np.int64)
    if g.ndim != 1 or g.shape != i.shape:
        raise ValueError(f"genuine_key and impostor_key must be 1-D of one length, got {g.shape} and {i.shape}")
    return g, i


def open_set_rates(genuine_key, impostor_key, metric, thresholds=None) -> OpenSetRates:
    """FNIR(t), FPIR(t) and the rank-1 accuracy from the leave-one-out keys (pure host).
    ``thresholds`` defaults to the sorted distinct finite scores of both sides."""
    metric = _metric_name(metric)
    g, i = _keys(genuine_key, impostor_key)
    has_g, has_i = g != N.EF_KEY_NONE, i != N.EF_KEY_NONE
    _, gs = decode_keys(g, metric)
    _, is_ = decode_keys(i, metric)
    gs, is_ = gs.astype(np.float64), is_.astype(np.float64)
    if thresholds is None:
        both = np.concatenate([gs[has_g], is_[has_i]])
        thresholds = np.unique(both[np.isfinite(both)])
    t = np.atleast_1d(np.asarray(thresholds, np.float64))
    correct = has_g & (g < i)
    rank1 = float(correct[has_g].mean()) if has_g.any() else float("nan")
    fnir = np.full(t.shape, np.nan)
    fpir = np.full(t.shape, np.nan)
    if has_g.any():
        hit = correct[has_g][None, :] & _accept(gs[has_g][None, :], t[:, None], metric)
        fnir = 1.0 - hit.mean(axis=1)
    if has_i.any():
        fpir = _accept(is_[has_i][None, :], t[:, None], metric).mean(axis=1)
    return OpenSetRates(t, fnir, fpir, rank1)


def equal_error_threshold(genuine_key, impostor_key, metric, thresholds=None) -> float:
    """The candidate threshold with the smallest max(FNIR, FPIR); among equals the strictest
    (the largest similarity, the smallest distance).  A side without probes (NaN) does not
    count; NaN when there is no candidate."""
    metric = _metric_name(metric)
    r = open_set_rates(genuine_key, impostor_key, metric, thresholds)
    if r.thresholds.size == 0:
        return float("nan")
    worst = np.fmax(r.fnir, r.fpir)
    if np.isnan(worst).all():
        return float("nan")
    tied = r.thresholds[worst == np.nanmin(worst)]
    return float(tied.max() if metric == "cosine" else tied.min())


def leave_one_out(G, labels, metric="cosine", device=0, batch=4096, engine=None):
    """Every row of the labelled gallery ``G`` (n, k) against all the others: loads G and its
    int32 ``labels`` into the engine (a new Engine(device) unless ``engine`` is given) and
    sends the rows through the SAME and the OTHER search with ``exclude_rows = arange``, in
    batches.  Returns a dict: genuine_key, impostor_key (int64) and their decoded rows and
    scores (genuine_idx, genuine_score, impostor_idx, impostor_score; -1 / NaN for none)."""
    from .engine import Engine
    metric = _metric_name(metric)
    g = np.ascontiguousarray(G, dtype=np.float32)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if g.ndim != 2 or lab.shape != (g.shape[0],):
        raise ValueError(f"G must be (n, k) and labels (n,), got {g.shape} and {lab.shape}")
    n = g.shape[0]
    own = engine is None
    e = Engine(device) if own else engine
    try:
        e.set_gallery(g)
        e.set_gallery_labels(lab)
        gk = np.empty(n, np.int64)
        ik = np.empty(n, np.int64)
        rows = np.arange(n, dtype=np.int64)
        for a in range(0, n, int(batch)):
            s = slice(a, min(n, a + int(batch)))
            gk[s] = e.search_labelled_keys(g[s], lab[s], "same", rows[s], metric)
            ik[s] = e.search_labelled_keys(g[s], lab[s], "other", rows[s], metric)
    finally:
        if own:
            e.close()
    gi, gs = decode_keys(gk, metric)
    ii, is_ = decode_keys(ik, metric)
    return {"genuine_key": gk, "impostor_key": ik, "genuine_idx": gi, "genuine_score": gs,
            "impostor_idx": ii, "impostor_score": is_}


def summarize(genuine_key, impostor_key, metric="cosine", thresholds=REFERENCE_THRESHOLDS):
    """The host half of evaluate_model: rank-1 accuracy, the equal-error threshold with its
    rates, and FNIR / FPIR at ``thresholds`` (the reference's 0.7 and 0.8 by default)."""
    metric = _metric_name(metric)
    eer_t = equal_error_threshold(genuine_key, impostor_key, metric)
    at = open_set_rates(genuine_key, impostor_key, metric, list(thresholds) + [eer_t])
    out = {"n": int(len(np.atleast_1d(genuine_key))), "metric": metric, "rank1": at.rank1,
           "equal_error_threshold": eer_t, "equal_error_fnir": float(at.fnir[-1]),
           "equal_error_fpir": float(at.fpir[-1]), "at": {}}
    for j, t in enumerate(thresholds):
        out["at"][float(t)] = {"fnir": float(at.fnir[j]), "fpir": float(at.fpir[j])}
    return out


def compare_subspaces(pca_features, fisher_features, labels, metric="l2", device=0, engine=None):
    """The same labelled rows in two feature spaces, side by side: ``{"pca": summarize(...),
    "fisher": summarize(...)}``, each from ``leave_one_out`` on its features.  What a
    discriminant fit (``Fisherfaces``) buys on the user's own gallery."""
    metric = _metric_name(metric)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    out = {}
    for name, feats in (("pca", pca_features), ("fisher", fisher_features)):
        loo = leave_one_out(feats, lab, metric, device, engine=engine)
        out[name] = summarize(loo["genuine_key"], loo["impostor_key"], metric)
    return out


def evaluate_model(model_data, metric="cosine", device=0, keys=None):
    """Leave-one-out evaluation of a model dict holding ``face_features`` (n, k) and
    ``face_labels`` (n,) — the face_model.pkl layout (train-v4.py:210-222).  Returns
    ``summarize``'s dict.  Labels of any type are mapped to int32 by value.  With one label
    only, the impostor side is empty and FPIR is NaN.  ``keys``: (genuine_key, impostor_key)
    computed earlier (leave_one_out); the GPU is then not touched."""
    feats = np.asarray(model_data["face_features"], np.float32)
    _, lab = np.unique(np.asarray(model_data["face_labels"]), return_inverse=True)
    if feats.ndim != 2 or lab.shape != (feats.shape[0],):
        raise ValueError(f"face_features must be (n, k) and face_labels (n,), got {feats.shape} and {lab.shape}")
    if keys is None:
        loo = leave_one_out(feats, lab.astype(np.int32), metric, device)
        keys = loo["genuine_key"], loo["impostor_key"]
    gk, ik = _keys(*keys)
    if gk.shape != (feats.shape[0],):
        raise ValueError(f"keys must hold one entry per gallery row ({feats.shape[0]}), got {gk.shape}")
    return summarize(gk, ik, metric)
