"""numpy reference of the gallery clustering (ef_gallery_cluster): fp64 pair scores from the fp32
features, the threshold graph, components by a plain union-find, the density rule with the
lowest-index core attachment, canonical numbering, and delta from the formula in
include/eigenface.h (never from the kernel's output)."""
import numpy as np

U = 2.0 ** -24


def kp_of(k):  # csrc/ef_internal.hpp feature_pad
    for p in (16, 32, 64, 128, 256, 512):
        if k <= p:
            return p
    return (k + 127) // 128 * 128


def pair_scores(g, metric, block=32, gram=False):
    """fp64 score of every row pair of the fp32 features g (n, k): the squared distance in
    difference form (l2; ``gram``: |a|^2 + |b|^2 - 2 a.b in fp64, for large n) or the cosine
    similarity, 0 for a zero row.  Non-finite rows give non-finite scores."""
    g = np.asarray(g, np.float32).astype(np.float64)
    n = g.shape[0]
    out = np.empty((n, n), np.float64)
    with np.errstate(all="ignore"):
        if metric == "l2":
            if gram:
                sq = (g * g).sum(axis=1)
                out[:] = sq[:, None] + sq[None, :] - 2.0 * (g @ g.T)
                np.fill_diagonal(out, 0.0)
            else:
                for a in range(0, n, block):
                    d = g[a:a + block, None, :] - g[None, :, :]
                    out[a:a + block] = (d * d).sum(axis=2)
        else:
            sq = (g * g).sum(axis=1)
            den = np.sqrt(sq)[:, None] * np.sqrt(sq)[None, :]
            out[:] = (g @ g.T) / den
            zero = sq == 0.0
            out[zero, :] = np.where(~np.isfinite(sq)[None, :], np.nan, 0.0)
            out[:, zero] = np.where(~np.isfinite(sq)[:, None], np.nan, 0.0)
    return out


def linked(scores, metric, t):
    """The threshold graph: a boolean (n, n) matrix without the diagonal; a pair whose score is not
    finite is never linked."""
    with np.errstate(invalid="ignore"):
        adj = (scores <= t) if metric == "l2" else (scores >= t)
    adj &= np.isfinite(scores)
    adj &= adj.T
    np.fill_diagonal(adj, False)
    return adj


def components(adj):
    """root[i] = the lowest row of i's connected component, by a union-find whose links point to
    the lower root."""
    n = adj.shape[0]
    parent = np.arange(n)
    for i in range(n):
        nb = np.flatnonzero(adj[i, i + 1:]) + i + 1
        if nb.size == 0:
            continue
        r = np.append(nb, i)
        while True:
            rr = parent[r]
            if (rr == r).all():
                break
            r = rr
        roots = np.unique(r)
        parent[roots] = roots[0]
    while True:
        pp = parent[parent]
        if (pp == parent).all():
            return parent
        parent = pp


def canonical(root, keep=None):
    """labels: the rank of each row's root among the roots, in row order (-1 where root < 0)."""
    root = np.asarray(root)
    roots = np.unique(root[root >= 0]) if keep is None else keep
    lab = np.full(root.shape[0], -1, np.int32)
    ok = root >= 0
    lab[ok] = np.searchsorted(roots, root[ok]).astype(np.int32)
    return lab


def reference(g, metric, t, min_samples=1, scores=None, gram=False):
    """(labels int32, degree int32, info int64[3]) as ef_gallery_cluster defines them."""
    s = pair_scores(g, metric, gram=gram) if scores is None else scores
    adj = linked(s, metric, t)
    n = adj.shape[0]
    degree = adj.sum(axis=1).astype(np.int32)
    core = degree + 1 >= min_samples if min_samples > 1 else np.ones(n, bool)
    root = components(adj & core[:, None] & core[None, :])
    final = np.where(core, root, -1)
    for r in np.flatnonzero(~core):
        nb = np.flatnonzero(adj[r] & core)
        if nb.size:
            final[r] = root[nb[0]]  # the lowest-index linked core row's cluster
    core_roots = np.flatnonzero(core & (root == np.arange(n)))
    labels = canonical(final, core_roots)
    info = np.array([core_roots.size, int((final < 0).sum()), int(adj.sum()) // 2], np.int64)
    return labels, degree, info


def delta(g, metric, scores=None):
    """The header's bound without the bin-index term, at the gallery's own maxima (q = g)."""
    g64 = np.asarray(g, np.float32).astype(np.float64)
    kp = kp_of(g64.shape[1])
    if metric != "l2":
        return 2.0 * (kp + 12) * U * 1.01
    with np.errstate(all="ignore"):
        sq = (g64 * g64).sum(axis=1)
    sq = sq[np.isfinite(sq)]
    gm2 = float(sq.max(initial=0.0))
    s = pair_scores(g, metric) if scores is None else scores
    smax = float(np.abs(s[np.isfinite(s)]).max(initial=0.0))
    return 2.0 * ((kp + 4) * U * 1.01 * (2.0 * gm2 + gm2) + 4.0 * U * smax)


def upper(scores):
    """The finite scores of the unordered pairs i < j, sorted."""
    v = scores[np.triu_indices(scores.shape[0], 1)]
    return np.sort(v[np.isfinite(v)])


def widest_gap(scores, lo, hi):
    """(t, half-width): the midpoint of the widest gap between neighbouring sorted pair scores
    that meets [lo, hi]."""
    v = upper(scores)
    a, b = v[:-1], v[1:]
    ok = (b >= lo) & (a <= hi) & (b > a)
    assert ok.any(), "no gap of the pair scores meets the window"
    i = np.flatnonzero(ok)[np.argmax((b - a)[ok])]
    return 0.5 * (v[i] + v[i + 1]), 0.5 * (v[i + 1] - v[i])


def blobs(n, k, ncls, seed, spread=4.0):
    """Class centres N(0, spread^2) per component plus unit noise; classes in random row order."""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, ncls, n)
    cls[:ncls] = np.arange(ncls)[:n]
    centres = spread * rng.standard_normal((ncls, k))
    g = (centres[cls] + rng.standard_normal((n, k))).astype(np.float32)
    return g, cls.astype(np.int32)
