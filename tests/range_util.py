"""numpy reference of the range search (ef_search_range): fp64 scores of probes against rows from
the fp32 features, block by block over the probes (never a b x n array for the large cases), the
hits as a CSR list in ascending row order, and delta per probe from the formula in
include/eigenface.h (never from the kernel's output)."""
import numpy as np

from cluster_util import U, kp_of


def block_scores(q, g, metric, gram=False):
    """fp64 score of every (probe, row) pair of the fp32 features q (m, k), g (n, k): the squared
    distance in difference form (l2; ``gram``: |q|^2 + |g|^2 - 2 q.g in fp64, exact for small
    integers) or the cosine similarity, 0 for a zero vector.  Non-finite rows or probes give
    non-finite scores."""
    q = np.asarray(q, np.float32).astype(np.float64)
    g = np.asarray(g, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if metric == "l2":
            if gram:
                return (q * q).sum(axis=1)[:, None] + (g * g).sum(axis=1)[None, :] - 2.0 * (q @ g.T)
            d = q[:, None, :] - g[None, :, :]
            return (d * d).sum(axis=2)
        qq, gg = (q * q).sum(axis=1), (g * g).sum(axis=1)
        out = (q @ g.T) / (np.sqrt(qq)[:, None] * np.sqrt(gg)[None, :])
        out[qq == 0.0, :] = np.where(~np.isfinite(gg)[None, :], np.nan, 0.0)
        out[:, gg == 0.0] = np.where(~np.isfinite(qq)[:, None], np.nan, 0.0)
        return out


def blocks(b, n, k, gram):
    """Probe block length that keeps a block's temporaries near 64 MB."""
    per = n * (8 if gram else 8 * k)
    return max(1, min(b, (64 << 20) // max(per, 1)))


def delta(q, g, metric, t):
    """delta_p of the header, one per probe (fp64): the band inside which the kernel settles a pair
    on its fp64 score."""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    g64 = np.asarray(g, np.float32).astype(np.float64)
    kp = kp_of(g64.shape[1])
    terr = abs(float(np.float32(t)) - float(t))
    if metric != "l2":
        return np.full(q64.shape[0], 2.0 * (kp + 12) * U * 1.01 + terr)
    with np.errstate(all="ignore"):
        gg = (g64 * g64).sum(axis=1)
        qn = np.sqrt((q64 * q64).sum(axis=1))
    gm2 = float(gg[np.isfinite(gg)].max(initial=0.0))
    gm = np.sqrt(gm2)
    return 2.0 * ((kp + 4) * U * 1.01 * (2.0 * qn * gm + gm2) + 4.0 * U * (qn + gm) ** 2) + terr


def accept(s, metric, t):
    with np.errstate(invalid="ignore"):
        hit = (s <= t) if metric == "l2" else (s >= t)
    return hit & np.isfinite(s)


def reference(q, g, metric, t, exclude=None, offset=0, gram=False):
    """(lims int64 (b + 1,), rows int64 global and ascending per probe, scores fp64) as
    ef_search_range defines the hits.  ``exclude``: global row per probe, anything outside
    [offset, offset + n) excludes nothing."""
    b, n = q.shape[0], g.shape[0]
    step = blocks(b, n, g.shape[1], gram)
    counts = np.zeros(b, np.int64)
    rows, scores = [], []
    for a in range(0, b, step):
        s = block_scores(q[a:a + step], g, metric, gram)
        hit = accept(s, metric, t)
        if exclude is not None:
            e = np.asarray(exclude[a:a + step], np.int64) - offset
            ok = (e >= 0) & (e < n)
            hit[np.flatnonzero(ok), e[ok]] = False
        p, r = np.nonzero(hit)  # row-major: probes in order, rows ascending inside a probe
        counts[a:a + step] = hit.sum(axis=1)
        rows.append(r.astype(np.int64) + offset)
        scores.append(s[p, r])
    lims = np.zeros(b + 1, np.int64)
    np.cumsum(counts, out=lims[1:])
    return lims, np.concatenate(rows) if rows else np.zeros(0, np.int64), \
        np.concatenate(scores) if scores else np.zeros(0, np.float64)


def brute_force(q, g, metric, t, exclude=None, offset=0):
    """The same by a plain double loop over the pairs (small inputs)."""
    q64, g64 = np.asarray(q, np.float64), np.asarray(g, np.float64)
    lims, rows, scores = [0], [], []
    for p in range(q64.shape[0]):
        for r in range(g64.shape[0]):
            if exclude is not None and exclude[p] == r + offset:
                continue
            with np.errstate(all="ignore"):
                if metric == "l2":
                    s = float(((q64[p] - g64[r]) ** 2).sum())
                else:
                    qq, gg = float((q64[p] ** 2).sum()), float((g64[r] ** 2).sum())
                    if np.isnan(qq) or np.isnan(gg) or np.isinf(qq) or np.isinf(gg):
                        s = float("nan")
                    elif qq == 0.0 or gg == 0.0:
                        s = 0.0
                    else:
                        s = float((q64[p] * g64[r]).sum()) / (np.sqrt(qq) * np.sqrt(gg))
            if np.isfinite(s) and (s <= t if metric == "l2" else s >= t):
                rows.append(r + offset)
                scores.append(s)
        lims.append(len(rows))
    return np.array(lims, np.int64), np.array(rows, np.int64), np.array(scores, np.float64)


def finite_scores(q, g, metric, gram=False):
    """All finite pair scores, sorted (small and medium inputs: b x n values)."""
    b = q.shape[0]
    step = blocks(b, g.shape[0], g.shape[1], gram)
    v = np.concatenate([block_scores(q[a:a + step], g, metric, gram).ravel() for a in range(0, b, step)])
    return np.sort(v[np.isfinite(v)])


def widest_gap(v, lo, hi):
    """(t, half-width): the midpoint of the widest gap between neighbouring sorted scores v that
    meets [lo, hi]."""
    a, b = v[:-1], v[1:]
    ok = (b >= lo) & (a <= hi) & (b > a)
    assert ok.any(), "no gap of the pair scores meets the window"
    i = np.flatnonzero(ok)[np.argmax((b - a)[ok])]
    return 0.5 * (v[i] + v[i + 1]), 0.5 * (v[i + 1] - v[i])


def no_score_at(v, t, scale=0.0):
    """An input condition: no pair within 1e-12 max(|t|, scale) of t, where two fp64 formulas
    could disagree.  v: the finite pair scores."""
    assert (np.abs(v - t) > 1e-12 * max(abs(t), scale, 1e-300)).all()
