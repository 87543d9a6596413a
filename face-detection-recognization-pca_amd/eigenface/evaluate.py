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


# ------------------------------------------------------------------- pairwise verification
# The score census (Engine.score_census, ef_score_census) counts ALL genuine and ALL impostor
# pair scores of a labelled gallery into two histograms on the GPU; everything below it is host
# arithmetic on those (2, nbins + 3) counts: slot 0 the scores below lo, slots 1 .. nbins the
# bins of width (hi - lo) / nbins, slot nbins + 1 the scores at or above hi, slot nbins + 2 the
# pairs whose score is not finite.

@dataclass
class VerificationRates:
    thresholds: np.ndarray  # the nbins + 1 bin edges lo + j (hi - lo) / nbins, ascending
    fmr: np.ndarray         # share of the impostor pairs accepted at each edge (NaN: no impostor pair)
    fnmr: np.ndarray        # share of the genuine pairs rejected at each edge (NaN: no genuine pair)
    metric: str
    n_genuine: int          # pairs with a finite score: the denominators
    n_impostor: int
    nonfinite: tuple        # (genuine, impostor) pairs whose score is not finite: in no rate


def _census_counts(counts):
    c = np.asarray(counts)
    if c.ndim != 2 or c.shape[0] != 2 or c.shape[1] < 4 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"counts must be an integer array (2, nbins + 3), got {c.dtype} {c.shape}")
    if (c < 0).any():
        raise ValueError("counts must not be negative")
    return c.astype(np.int64), c.shape[1] - 3


def _census_range(lo, hi):
    lo, hi = float(lo), float(hi)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"the range must be finite with lo < hi, got ({lo}, {hi})")
    return lo, hi


def verification_rates(counts, lo, hi, metric) -> VerificationRates:
    """FMR and FNMR at the nbins + 1 bin edges from the census counts (pure host).  A pair is
    accepted at edge e when it is binned on the accepting side of e (``_accept``'s direction):
    score >= e for cosine, score < e for L2 (<= but for the scores equal to an edge, which the
    bins cannot tell).  The non-finite slot is in no numerator and no denominator; a side
    without a finite pair gives NaN."""
    metric = _metric_name(metric)
    c, nbins = _census_counts(counts)
    lo, hi = _census_range(lo, hi)
    edges = lo + (hi - lo) * np.arange(nbins + 1, dtype=np.float64) / nbins
    finite = c[:, :nbins + 2]
    below = np.cumsum(finite, axis=1)[:, :nbins + 1]  # binned below edge j: slots 0 .. j
    total = finite.sum(axis=1)
    accepted = total[:, None] - below if metric == "cosine" else below
    with np.errstate(invalid="ignore", divide="ignore"):
        share = np.where(total[:, None] > 0, accepted / np.maximum(total[:, None], 1).astype(np.float64), np.nan)
    return VerificationRates(edges, share[1], 1.0 - share[0], metric, int(total[0]), int(total[1]),
                             (int(c[0, nbins + 2]), int(c[1, nbins + 2])))


def pair_equal_error(rates: VerificationRates):
    """(threshold, rate): the edge with the smallest max(FMR, FNMR) and that maximum; among equals
    the strictest edge (the largest similarity, the smallest distance), equal_error_threshold's
    rule.  A side without pairs (NaN) does not count; (NaN, NaN) when neither has any."""
    worst = np.fmax(rates.fmr, rates.fnmr)
    if worst.size == 0 or np.isnan(worst).all():
        return float("nan"), float("nan")
    best = np.nanmin(worst)
    tied = rates.thresholds[worst == best]
    return float(tied.max() if rates.metric == "cosine" else tied.min()), float(best)


def tar_at_fmr(rates: VerificationRates, fmr) -> float:
    """The largest true-accept rate 1 - FNMR over the edges whose FMR is at most ``fmr``; NaN when
    no edge qualifies or a side has no pairs."""
    ok = rates.fmr <= float(fmr)  # False for NaN
    tar = (1.0 - rates.fnmr)[ok]
    tar = tar[~np.isnan(tar)]
    return float(tar.max()) if tar.size else float("nan")


def auc(rates: VerificationRates) -> float:
    """Area under the ROC (FMR, TAR) through the edges, closed at (0, 0) and (1, 1), by the
    trapezoid rule; NaN when a side has no pairs."""
    if np.isnan(rates.fmr).any() or np.isnan(rates.fnmr).any():
        return float("nan")
    x = np.concatenate([[0.0], rates.fmr, [1.0]])
    y = np.concatenate([[0.0], 1.0 - rates.fnmr, [1.0]])
    order = np.lexsort((y, x))
    x, y = x[order], y[order]
    return float(((x[1:] - x[:-1]) * (y[1:] + y[:-1])).sum() / 2.0)


def d_prime(counts, lo, hi) -> float:
    """|mean_g - mean_i| / sqrt((var_g + var_i) / 2) from the bin centres, weighted by the counts
    of the nbins inner bins (the outer and the non-finite slots have no centre and are left
    out).  NaN when a side has no pair inside the range or both variances vanish at one mean."""
    c, nbins = _census_counts(counts)
    lo, hi = _census_range(lo, hi)
    centre = lo + (hi - lo) * (np.arange(nbins, dtype=np.float64) + 0.5) / nbins
    w = c[:, 1:nbins + 1].astype(np.float64)
    tot = w.sum(axis=1)
    if (tot == 0).any():
        return float("nan")
    mean = (w * centre).sum(axis=1) / tot
    var = (w * (centre[None, :] - mean[:, None]) ** 2).sum(axis=1) / tot
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(abs(mean[0] - mean[1]) / np.sqrt((var[0] + var[1]) / 2.0))


def _default_census_range(g, metric):
    if metric == "cosine":
        return -1.0, 1.0  # a similarity that rounds to >= 1 falls in the top slot, an outer bin of the rates
    top = 4.0 * float((np.asarray(g, np.float64) ** 2).sum(axis=1).max(initial=0.0))  # ||a - b||^2 <= 4 max ||g||^2
    hi = np.float32(top)
    if float(hi) < top:
        hi = np.nextafter(hi, np.float32(np.inf))
    return 0.0, float(hi) if hi > 0 and np.isfinite(hi) else 1.0


def score_census(G, labels, metric="cosine", nbins=1024, range=None, device=0, batch=4096, engine=None):
    """The census of a labelled gallery against itself, leave-one-out: every row of ``G`` (n, k)
    is a probe, its own row is excluded, and the batches' counts are summed on the host.  Loads G
    and its int32 ``labels`` into the engine (a new Engine(device) unless ``engine`` is given).
    Returns ``(counts, (lo, hi))``: counts int64 (2, nbins + 3), genuine then impostor, and the
    float32 range they were binned over — by default (-1, 1) for cosine and (0, 4 max ||g||^2)
    for L2, the maximum taken from the data in fp64.  Every unordered pair {a, b} appears twice,
    as (a, b) and as (b, a): the counts are of ordered pairs, which leaves every rate unchanged."""
    from .engine import Engine
    metric = _metric_name(metric)
    g = np.ascontiguousarray(G, dtype=np.float32)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    if g.ndim != 2 or lab.shape != (g.shape[0],):
        raise ValueError(f"G must be (n, k) and labels (n,), got {g.shape} and {lab.shape}")
    lo, hi = _default_census_range(g, metric) if range is None else range
    lo, hi = _census_range(np.float32(lo), np.float32(hi))
    nbins = int(nbins)
    n = g.shape[0]
    own = engine is None
    e = Engine(device) if own else engine
    try:
        e.set_gallery(g)
        e.set_gallery_labels(lab)
        counts = np.zeros((2, nbins + 3), np.int64)
        rows = np.arange(n, dtype=np.int64)
        for a in np.arange(0, n, int(batch)):
            s = slice(int(a), min(n, int(a) + int(batch)))
            counts += e.score_census(g[s], lab[s], rows[s], metric, nbins, (lo, hi))
    finally:
        if own:
            e.close()
    return counts, (lo, hi)


def summarize_verification(counts, lo, hi, metric, fmr=(1e-2, 1e-3)):
    """The host half of compare_verification: pair counts, the pairwise equal-error threshold and
    rate, AUC, d' and the true-accept rate at each target FMR."""
    r = verification_rates(counts, lo, hi, metric)
    t, eer = pair_equal_error(r)
    return {"metric": r.metric, "range": (float(lo), float(hi)), "n_genuine": r.n_genuine, "n_impostor": r.n_impostor,
            "nonfinite": r.nonfinite, "equal_error_threshold": t, "equal_error_rate": eer, "auc": auc(r),
            "d_prime": d_prime(counts, lo, hi), "tar_at_fmr": {float(f): tar_at_fmr(r, f) for f in fmr}}


def compare_verification(pca_features, fisher_features, labels, metric="l2", fmr=(1e-2, 1e-3), nbins=1024, device=0,
                         batch=4096, engine=None):
    """The pairwise counterpart of compare_subspaces: the same labelled rows in two feature
    spaces, ``{"pca": summarize_verification(...), "fisher": ...}``, each from ``score_census`` on
    its features over its own default range.  What a discriminant fit buys at a fixed FMR."""
    metric = _metric_name(metric)
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    out = {}
    for name, feats in (("pca", pca_features), ("fisher", fisher_features)):
        counts, (lo, hi) = score_census(feats, lab, metric, nbins, None, device, batch, engine)
        out[name] = summarize_verification(counts, lo, hi, metric, fmr)
    return out


def clustering_agreement(labels_true, labels_pred):
    """How well a clustering (``cluster_gallery``'s labels; -1 = noise, each a cluster of its own)
    recovers known identities: the integer pair counts and pair precision, recall and F1
    (``cluster.pair_confusion`` / ``pairwise_scores``; host arithmetic, no GPU)."""
    from .cluster import pair_confusion, pairwise_scores
    tp, fp, fn, tn = pair_confusion(labels_true, labels_pred)
    return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, **pairwise_scores(labels_true, labels_pred)}


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


# ------------------------------------------------------------------- identification rank
# Engine.search_rank (ef_search_rank) gives, per probe, ``better``: the number of other identities
# that come before the probe's own, -1 for a probe without a genuine row.  The rank is better + 1;
# everything below is host arithmetic on that array.

def _better(better):
    b = np.asarray(better)
    if b.ndim != 1 or not np.issubdtype(b.dtype, np.integer):
        raise ValueError(f"better must be a 1-D integer array, got {b.dtype} {b.shape}")
    if (b < -1).any():
        raise ValueError("better must be -1 (no genuine row) or a count")
    return b.astype(np.int64)


def cmc_curve(better, max_rank=None):
    """The cumulative match characteristic: ``(ranks 1 .. R, share of the probes with a genuine
    row whose rank better + 1 is <= r)``.  R defaults to the largest rank present (1 when there is
    none).  Probes without a genuine row (-1) are in no numerator and no denominator; the shares are
    NaN when no probe has one."""
    b = _better(better)
    ranks = b[b >= 0] + 1
    if max_rank is None:
        max_rank = int(ranks.max()) if ranks.size else 1
    R = int(max_rank)
    if R < 1:
        raise ValueError(f"max_rank must be >= 1, got {max_rank}")
    r = np.arange(1, R + 1)
    if ranks.size == 0:
        return r, np.full(R, np.nan)
    hist = np.bincount(np.minimum(ranks, R + 1), minlength=R + 2)[1:R + 1]
    return r, np.cumsum(hist) / ranks.size


def mean_reciprocal_rank(better):
    """Mean of 1 / rank over the probes with a genuine row; NaN when there is none."""
    b = _better(better)
    ranks = b[b >= 0] + 1
    return float(np.mean(1.0 / ranks)) if ranks.size else float("nan")


def summarize_identification(better, ranks=(1, 5, 10, 20)):
    """Rank-r identification rates at ``ranks``, the mean reciprocal rank, the median and the
    largest rank, and the probe counts: ``{"n", "n_genuine", "rank": {r: rate}, "mrr",
    "median_rank", "max_rank"}`` (NaN / None where no probe has a genuine row)."""
    b = _better(better)
    rk = b[b >= 0] + 1
    out = {"n": int(b.size), "n_genuine": int(rk.size), "rank": {}, "mrr": mean_reciprocal_rank(b),
           "median_rank": float(np.median(rk)) if rk.size else float("nan"),
           "max_rank": int(rk.max()) if rk.size else None}
    for r in ranks:
        if int(r) < 1:
            raise ValueError(f"ranks must be >= 1, got {r}")
        out["rank"][int(r)] = float((rk <= int(r)).mean()) if rk.size else float("nan")
    return out


def identification_ranks(G, labels, metric="cosine", device=0, batch=4096, engine=None):
    """The leave-one-out form of ``Engine.search_rank``: every row of the labelled gallery ``G``
    (n, k) against all the others (``exclude_rows = arange``), in batches, as ``leave_one_out``
    runs the labelled search.  Returns ``better`` int32 (n,): feed it to ``cmc_curve`` /
    ``summarize_identification``."""
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
        better = np.empty(n, np.int32)
        rows = np.arange(n, dtype=np.int64)
        for a in range(0, n, int(batch)):
            s = slice(a, min(n, a + int(batch)))
            better[s] = e.search_rank(g[s], lab[s], rows[s], metric)[0]
    finally:
        if own:
            e.close()
    return better


def search_rank_plan(b, n, n_classes, bitmap_bytes=256 << 20):
    """ef_search_rank_plan (host only): ``(words_per_probe, probes_per_piece, n_pieces)`` of a rank
    search with b probes over n rows of n_classes identities under a bitmap budget."""
    import ctypes as C
    w, p, m = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    rc = N.lib().ef_search_rank_plan(int(b), int(n), int(n_classes), int(bitmap_bytes), C.byref(w), C.byref(p),
                                     C.byref(m))
    if rc != N.EF_OK:
        raise N.EigenfaceError(rc, "ef_search_rank_plan: bad arguments")
    return int(w.value), int(p.value), int(m.value)
