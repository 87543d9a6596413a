"""numpy reference of the gallery clustering (ef_gallery_cluster): fp64 pair scores from the fp32
features, the threshold graph, components by a plain union-find, the density rule with the
lowest-index core attachment, canonical numbering, and delta from the formula in
include/eigenface.h (never from the kernel's output).  For galleries too large for an n x n
array: an integer lattice whose exact answer comes from a dict of its occupied points."""
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


def delta(g, metric, scores=None, from_norms=False):
    """The header's bound without the bin-index term, at the gallery's own maxima (q = g).
    ``from_norms``: |s| <= 4 max|g|^2 stands in for the largest pair score (the call's own form),
    so that no n x n array is needed."""
    g64 = np.asarray(g, np.float32).astype(np.float64)
    kp = kp_of(g64.shape[1])
    if metric != "l2":
        return 2.0 * (kp + 12) * U * 1.01
    with np.errstate(all="ignore"):
        sq = (g64 * g64).sum(axis=1)
    sq = sq[np.isfinite(sq)]
    gm2 = float(sq.max(initial=0.0))
    if from_norms:
        smax = 4.0 * gm2
    else:
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


# ------------------------------------------------------------------ the lattice gallery
def lattice(n, k, seed, ngroups=None):
    """Integer-valued fp32 rows (n, k >= 8) whose threshold graph is known without an n x n array.
    Coordinates 0 .. 5 hold the base-8 digits of the row's group id as 4 digit + 1, coordinates
    6 and 7 are 0 or 1, the rest are the constant 3; the groups (n // 3 distinct random ids unless
    ``ngroups`` says otherwise) are dealt to the rows at random, so a group's members lie in
    tiles far apart.  Squared distances are exact integers in fp32: 0, 1, 1 or 2 inside a group,
    at least 16 between groups."""
    assert k >= 8
    rng = np.random.default_rng(seed)
    ngroups = max(1, n // 3) if ngroups is None else ngroups
    ids = rng.choice(8 ** 6, ngroups, replace=False)[rng.integers(0, ngroups, n)]
    g = np.full((n, k), 3.0, np.float32)
    for c in range(6):
        g[:, c] = 4 * ((ids >> (3 * c)) & 7) + 1
    g[:, 6:8] = rng.integers(0, 2, (n, 2))
    return g


def _row_keys(p):
    """One bytes object per row of the 2-D integer array p."""
    p = np.ascontiguousarray(p)
    return p.view(np.dtype((np.void, p.shape[1] * p.itemsize))).ravel().tolist()


def lattice_cells(g):
    """The occupied points of an integer-valued gallery: (cell of each row, rows of each cell in
    ascending order, pairs (c, c2) of occupied cells one unit step apart, each once).  A dict
    from point to cell; the 2 k unit neighbours of a cell are looked up in it."""
    p = np.rint(np.asarray(g, np.float64)).astype(np.int32)
    assert (p == g).all() and np.abs(p).max() < 2 ** 11  # integers; |g|^2 and every partial sum exact in fp32
    index, members = {}, []
    cell = np.empty(p.shape[0], np.int64)
    for i, key in enumerate(_row_keys(p)):
        c = index.setdefault(key, len(members))
        if c == len(members):
            members.append([])
        members[c].append(i)
        cell[i] = c
    pts = p[[m[0] for m in members]]
    steps = []
    for j in range(p.shape[1]):  # the neighbour one step up in coordinate j; the step down is its mirror
        up = pts.copy()
        up[:, j] += 1
        for c, key in enumerate(_row_keys(up)):
            c2 = index.get(key)
            if c2 is not None:
                steps.append((c, c2))
    return cell, members, np.array(steps, np.int64).reshape(-1, 2)


def lattice_reference(g, min_samples=1, unit_steps=True):
    """(labels int32, degree int32, info int64[3]) as ``reference`` gives them for L2 at t = 1.0 on
    an integer-valued gallery, in O(n k): two rows link iff they are the same point or one unit
    step apart.  ``unit_steps`` False: only rows at the same point link (the duplicates)."""
    cell, members, steps = lattice_cells(g)
    if not unit_steps:
        steps = steps[:0]
    n, m = cell.shape[0], len(members)
    occ = np.array([len(r) for r in members], np.int64)
    first = np.array([r[0] for r in members], np.int64)
    around = np.zeros(m, np.int64)  # rows in the cells one step away
    np.add.at(around, steps[:, 0], occ[steps[:, 1]])
    np.add.at(around, steps[:, 1], occ[steps[:, 0]])
    cdeg = occ - 1 + around  # every row of a cell has the cell's degree
    ccore = cdeg + 1 >= min_samples if min_samples > 1 else np.ones(m, bool)
    parent = np.arange(m)

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c
    for a, b in steps:
        if ccore[a] and ccore[b]:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    comp = np.array([find(c) for c in range(m)])
    lowest = np.full(m, n, np.int64)  # by component: its lowest core row
    np.minimum.at(lowest, comp[ccore], first[ccore])
    # a non-core cell: its rows take the cluster of the lowest core row one step away (the rows
    # at its own point are non-core like itself)
    nearest = np.full(m, n, np.int64)
    for a, b in ((0, 1), (1, 0)):
        ok = ccore[steps[:, b]] & ~ccore[steps[:, a]]
        np.minimum.at(nearest, steps[ok, a], first[steps[ok, b]])
    croot = np.where(ccore, lowest[comp], -1)
    att = ~ccore & (nearest < n)
    croot[att] = lowest[comp[cell[nearest[att]]]]
    final = croot[cell]
    core_roots = np.unique(lowest[comp[ccore]])
    labels = canonical(final, core_roots)
    links = int((occ * (occ - 1) // 2).sum() + (occ[steps[:, 0]] * occ[steps[:, 1]]).sum())
    info = np.array([core_roots.size, int((final < 0).sum()), links], np.int64)
    return labels, cdeg[cell].astype(np.int32), info


def lattice_unit_pairs(g):
    """Unordered row pairs at squared distance exactly 1."""
    _, members, steps = lattice_cells(g)
    occ = np.array([len(r) for r in members], np.int64)
    return int((occ[steps[:, 0]] * occ[steps[:, 1]]).sum())


def max_cosine_between_points(g, block=1024):
    """The largest fp64 cosine similarity of two rows that are not the same point, block by block
    over the distinct points (never an n x n array)."""
    pts = np.unique(np.asarray(g, np.float64), axis=0)
    u = pts / np.sqrt((pts * pts).sum(axis=1))[:, None]
    best = -1.0
    for a in range(0, u.shape[0], block):
        c = u[a:a + block] @ u[a:].T  # the upper triangle is enough
        r = np.arange(c.shape[0])
        c[r, r] = -1.0  # a point with itself
        best = max(best, float(c.max()))
    return best
