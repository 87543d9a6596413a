"""numpy reference of the identification rank (ef_search_rank): fp64 scores by range_util's
formulas from the fp32 features, the genuine row and its score tau per probe, the best score of
every other identity, ``better`` by the header's definition (exclusion, first-index ties, -1),
and delta per probe from the header's formula (never from the kernel)."""
import numpy as np

from cluster_util import U, kp_of
from range_util import block_scores


def scores64(q, g, metric, gram=False):
    """(b, n) fp64 scores as ef_match.score carries them: the squared distance, or the NEGATED
    cosine similarity: lower is better under both metrics."""
    s = block_scores(q, g, metric, gram)
    return s if metric == "l2" else -s


def reference(q, g, labels, plabels, metric, exclude=None, offset=0, gram=False, genuine=None):
    """dict of per-probe arrays as ef_search_rank defines them on this gallery (rows at global
    index offset + local):
      better   int32, -1 without a genuine row or with a tau that is not finite
      row_gen  int64 global index of the genuine row, -1 for none
      tau      fp64 score of the genuine row (NaN for none)
      margin   min over the other identities of |best score of the identity - tau| (inf: none)
      best     (b, C) best finite qualifying score per distinct label (inf: none), labels sorted
    ``genuine`` = (row_gen global, tau): the EF_RANK_GENUINE_GIVEN form; a row inside this shard has
    its tau recomputed here, a row outside keeps the given one; row_gen < 0 is "no record"."""
    labels = np.asarray(labels, np.int64)
    plabels = np.asarray(plabels, np.int64)
    b, n = q.shape[0], g.shape[0]
    s = scores64(q, g, metric, gram)
    ok = np.isfinite(s)
    if exclude is not None:
        e = np.asarray(exclude, np.int64) - offset
        inside = (e >= 0) & (e < n)
        ok[np.flatnonzero(inside), e[inside]] = False
    uniq = np.unique(labels)
    better = np.full(b, -1, np.int32)
    row_gen = np.full(b, -1, np.int64)
    tau = np.full(b, np.nan)
    margin = np.full(b, np.inf)
    best = np.full((b, uniq.size), np.inf)
    rows = np.arange(n, dtype=np.int64) + offset
    for p in range(b):
        if genuine is None:
            same = ok[p] & (labels == plabels[p])
            if not same.any():
                continue
            sp = np.where(same, s[p], np.inf)
            r = int(np.argmin(sp))  # the first index among equal scores
            row_gen[p], tau[p] = r + offset, s[p, r]
        else:
            if genuine[0][p] < 0:
                continue
            row_gen[p] = genuine[0][p]
            loc = row_gen[p] - offset
            tau[p] = s[p, loc] if 0 <= loc < n else genuine[1][p]
        if not np.isfinite(tau[p]):
            continue
        other = ok[p] & (labels != plabels[p])
        beats = other & ((s[p] < tau[p]) | ((s[p] == tau[p]) & (rows < row_gen[p])))
        better[p] = np.unique(labels[beats]).size
        so = np.where(other, s[p], np.inf)
        for c, lab in enumerate(uniq):
            if lab != plabels[p]:
                m = so[labels == lab]
                best[p, c] = m.min() if m.size else np.inf
        fin = best[p][np.isfinite(best[p])]
        if fin.size:
            margin[p] = np.abs(fin - tau[p]).min()
    return {"better": better, "row_gen": row_gen, "tau": tau, "margin": margin, "best": best, "scores": s, "ok": ok}


def largest_score(ref):
    v = ref["scores"][np.isfinite(ref["scores"])]
    return float(np.abs(v).max()) if v.size else 0.0


def clear_margins(ref, rel=1e-9, exact=()):
    """The default input condition: for every probe with a genuine row and every other identity,
    |best_c - tau_p| exceeds ``rel`` of the largest score, so a last-ulp difference between the
    numpy formula and the kernel's fp64 score cannot change a decision.  Also: the genuine row is
    not within that distance of another row of its identity, unless exactly equal (the labelled
    search's own tie tolerance is far below it).  ``exact``: probes whose scores are exact here and
    on the GPU (a zero probe under cosine), where a margin of exactly 0 is a tie both decide alike."""
    big = largest_score(ref)
    has = ref["better"] >= 0
    for p in exact:
        assert (ref["margin"][p] == 0.0) or (ref["margin"][p] > rel * big)
    has[list(exact)] = False
    assert (ref["margin"][has] > rel * big).all(), float(ref["margin"][has].min() / max(big, 1e-300))
    return float(ref["margin"][has].min() / big) if has.any() and big > 0 else np.inf


def delta(q, g, metric, tau):
    """delta_p of the header (fp64), one per probe: ef_search_range's formula with
    |fp32(tau_p) - tau_p| as the threshold's rounding term."""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    kp = kp_of(g64.shape[1])
    with np.errstate(all="ignore"):
        terr = np.abs(np.asarray(tau, np.float64).astype(np.float32).astype(np.float64) - tau)
        if metric != "l2":
            return 2.0 * (kp + 12) * U * 1.01 + terr
        gg = (g64 * g64).sum(axis=1)
        qn = np.sqrt((q64 * q64).sum(axis=1))
    gm2 = float(gg[np.isfinite(gg)].max(initial=0.0))
    gm = np.sqrt(gm2)
    return 2.0 * ((kp + 4) * U * 1.01 * (2.0 * qn * gm + gm2) + 4.0 * U * (qn + gm) ** 2) + terr


def settled_bounds(ref, d):
    """(lo, hi) on the pairs the call settles in fp64 (info[0]), from delta_p = 2 E + terr with E the
    bound on one scan score's error.  A qualifying finite pair of a probe with a genuine row whose
    fp64 score equals tau (the genuine pair itself, an exact tie) has a scan score within E + terr
    of fp32(tau): surely inside the band.  A pair with |s - tau| > 2 delta has one further than
    delta from it: surely outside."""
    has = ref["better"] >= 0
    dist = np.abs(ref["scores"] - ref["tau"][:, None])
    inband = ref["ok"] & has[:, None]
    lo = int((inband & (dist == 0.0)).sum())
    hi = int((inband & (dist <= 2.0 * np.asarray(d)[:, None])).sum())
    return lo, hi


def blobs(n, k, C, seed, sigma_c=3.5):
    """n rows of k components around C centres N(0, (sigma_c / sqrt(k))^2) with unit noise,
    identities interleaved in row order (row i belongs to identity i mod C), every identity
    present; labels are the identity numbers scattered over int32."""
    assert n >= C
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, k)) * (sigma_c / np.sqrt(k))
    ident = np.arange(n) % C
    g = (centres[ident] + rng.standard_normal((n, k))).astype(np.float32)
    names = np.sort(rng.choice(np.arange(-2 ** 20, 2 ** 20), C, replace=False)).astype(np.int32)
    rng.shuffle(names)
    return g, names[ident], centres, names


def better_blocked(q, g, labels, plabels, metric, exclude=None, offset=0, gram=False, block=1024):
    """``reference``'s better and row_gen without its loop over the probes, block by block (large
    inputs), and the local rows that beat some probe's genuine row (a boolean (n,))."""
    labels = np.asarray(labels, np.int64)
    plabels = np.asarray(plabels, np.int64)
    b, n = q.shape[0], g.shape[0]
    order = np.argsort(labels, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(labels[order]) != 0])
    rows = np.arange(n, dtype=np.int64) + offset
    better = np.full(b, -1, np.int32)
    row_gen = np.full(b, -1, np.int64)
    beating = np.zeros(n, bool)
    for a in range(0, b, block):
        s = scores64(q[a:a + block], g, metric, gram)
        m = s.shape[0]
        ok = np.isfinite(s)
        if exclude is not None:
            e = np.asarray(exclude[a:a + block], np.int64) - offset
            inside = (e >= 0) & (e < n)
            ok[np.flatnonzero(inside), e[inside]] = False
        same = labels[None, :] == plabels[a:a + block, None]
        sp = np.where(ok & same, s, np.inf)
        r = np.argmin(sp, axis=1)
        tau = sp[np.arange(m), r]
        has = np.isfinite(tau)
        gen = r + offset
        beats = ok & ~same & has[:, None] & ((s < tau[:, None]) | ((s == tau[:, None]) & (rows[None, :] < gen[:, None])))
        marked = np.add.reduceat(beats[:, order].astype(np.int32), starts, axis=1) > 0
        better[a:a + block] = np.where(has, marked.sum(axis=1), -1)
        row_gen[a:a + block] = np.where(has, gen, -1)
        beating |= beats.any(axis=0)
    return better, row_gen, beating
