"""What the search engine guarantees, as test assertions.

The engine resolves every probe's arg-best in fp64 (ef_search.hip reduce_kernel /
resolve_kernel): the returned row is the lowest index among the rows whose fp64 score is
within 1e-12 * (|best| + scale) of the best, with scale = ||q||^2 + max ||g||^2 for L2 and,
for cosine, scores -cos(q, g) (ef_search_common.hpp score64) with scale 1.  So:

* every probe whose fp64 top-2 gap exceeds that window must get exactly the oracle's
  first-arg-best row (np.argmin / np.argmax semantics) — no fraction floor;
* every other probe must get a row inside the window.

The checker scores in fp64 with the expanded form (||q||^2 + ||g||^2 - 2 q.g, or unit-row
dot products for cosine); its evaluation error is ~1e-15 of the scale, 1000x below the
window, so the 1.1x margin on the window absorbs it.
"""
import numpy as np

from oracle import eigenface_oracle as orc

WINDOW = 1e-12
MARGIN = 1.1


def top2(q, g, metric, chunk_rows=131072, chunk_probes=512):
    """fp64 (first-best index, best, runner-up) per probe over all gallery rows, scores as
    'smaller is better' (L2: squared distance; cosine: -cos in unit terms)."""
    q64 = np.asarray(q, np.float64)
    b = len(q64)
    idx = np.zeros(b, np.int64)
    best = np.full(b, np.inf)
    second = np.full(b, np.inf)
    if metric == "cosine":
        q64 = orc._unit_rows(q64)
    for p0 in range(0, b, chunk_probes):
        qs = q64[p0:p0 + chunk_probes]
        qq = (qs ** 2).sum(1)
        bi, bb, bs = idx[p0:p0 + chunk_probes], best[p0:p0 + chunk_probes], second[p0:p0 + chunk_probes]
        for a in range(0, len(g), chunk_rows):
            g64 = np.asarray(g[a:a + chunk_rows], np.float64)
            if metric == "l2":
                s = qq[:, None] + (g64 ** 2).sum(1)[None, :] - 2.0 * (qs @ g64.T)
            else:
                s = -(qs @ orc._unit_rows(g64).T)
            j = np.argmin(s, axis=1)  # first minimum inside the chunk
            cb = s[np.arange(len(qs)), j]
            if s.shape[1] > 1:
                s[np.arange(len(qs)), j] = np.inf
                c2 = s.min(axis=1)
            else:
                c2 = np.full(len(qs), np.inf)
            new = cb < bb  # strictly better: earlier chunks keep exact ties (first index)
            bs[:] = np.where(new, np.minimum(bb, c2), np.minimum(bs, cb))
            bi[:] = np.where(new, a + j, bi)
            bb[:] = np.where(new, cb, bb)
    return idx, best, second


def gmax2_of(g, chunk=131072):
    return max(((np.asarray(g[a:a + chunk], np.float64) ** 2).sum(1).max() for a in range(0, len(g), chunk)),
               default=0.0)


def window(q, g, metric, best, gmax2=None):
    """The engine's tie window per probe, in the checker's units."""
    q64 = np.asarray(q, np.float64)
    qn2 = (q64 ** 2).sum(1)
    if metric == "l2":
        scale = qn2 + (gmax2_of(g) if gmax2 is None else gmax2)
        return WINDOW * (np.abs(best) + scale)
    # cosine: resolve_kernel's fp64 score is -cos (score64: -q.g / (|q| |g|)), window
    # 1e-12 (|score| + 1)
    return WINDOW * (np.abs(best) + 1.0)


def chosen_scores(q, g, idx, metric):
    """fp64 scores of the rows the engine chose (same units as top2)."""
    q64 = np.asarray(q, np.float64)
    gi = np.asarray(g[idx], np.float64)
    if metric == "l2":
        return ((q64 - gi) ** 2).sum(1)
    return -(orc._unit_rows(q64) * orc._unit_rows(gi)).sum(1)


def assert_exact_argbest(q, g, idx, metric, ref=None, min_clear=None, gmax2=None):
    """The guarantee above.  ref: precomputed top2(q, g, metric).  Returns the boolean
    mask of probes outside the tie window (asserted exact)."""
    ref_idx, best, second = ref if ref is not None else top2(q, g, metric)
    idx = np.asarray(idx)
    w = MARGIN * window(q, g, metric, best, gmax2)
    mine = chosen_scores(q, g, idx, metric)
    bad = ~(mine - best <= w)
    assert not bad.any(), f"{metric}: {bad.sum()} probes chose a row outside the tie window " \
                          f"(first {np.flatnonzero(bad)[:5]})"
    clear = (second - best) > w
    miss = clear & (idx != ref_idx)
    assert not miss.any(), f"{metric}: {miss.sum()} of {clear.sum()} clear probes differ from the fp64 " \
                           f"first-arg-best (first {np.flatnonzero(miss)[:5]})"
    if min_clear is not None:
        assert clear.mean() >= min_clear, clear.mean()
    return clear


def top2_device(q, g, metric, chunk_rows=131072):
    """top2 with torch fp64 GEMMs on the GPU: an independent fp64 checker (rocBLAS, not
    the engine's kernels) for full-size batches the host cannot score in seconds
    (4096 probes x 1M rows).  Same units and semantics as top2 outside ties."""
    import torch
    dev = torch.device("cuda")
    q64 = torch.as_tensor(np.asarray(q), device=dev).double()
    if metric == "cosine":
        q64 = q64 / q64.norm(dim=1, keepdim=True).clamp_min(1e-300)
    qq = (q64 * q64).sum(1)
    b = q64.shape[0]
    best = torch.full((b,), float("inf"), dtype=torch.float64, device=dev)
    second = best.clone()
    idx = torch.zeros(b, dtype=torch.int64, device=dev)
    for a in range(0, len(g), chunk_rows):
        gc = g[a:a + chunk_rows]
        g64 = (gc if isinstance(gc, torch.Tensor) else torch.as_tensor(np.asarray(gc))).to(dev).double()
        if metric == "l2":
            s = qq[:, None] + (g64 * g64).sum(1)[None, :] - 2.0 * (q64 @ g64.T)
        else:
            s = -(q64 @ (g64 / g64.norm(dim=1, keepdim=True).clamp_min(1e-300)).T)
        if s.shape[1] > 1:
            v, j = torch.topk(s, 2, dim=1, largest=False)
            cb, c2, cj = v[:, 0], v[:, 1], j[:, 0]
        else:
            cb, c2, cj = s[:, 0], torch.full_like(s[:, 0], float("inf")), torch.zeros(b, dtype=torch.int64, device=dev)
        new = cb < best
        second = torch.where(new, torch.minimum(best, c2), torch.minimum(second, cb))
        idx = torch.where(new, a + cj, idx)
        best = torch.where(new, cb, best)
        del s
    return idx.cpu().numpy(), best.cpu().numpy(), second.cpu().numpy()


def plant_rivals(G, q, anchors, seed, avoid=()):
    """Near-tie stress: for probe i, a copy of gallery row anchors[i] whose
    coordinate of largest |q - g| is moved by 1..64 ulps (random direction), written over a
    row in the other half of the gallery (a different chunk).  Its fp64 score differs from
    the anchor's by ~1e-10..1e-7 of the scale: far inside fp32 (and bf16) rounding of the
    scan scores, far outside the 1e-12 tie window.  Returns (G2, rival rows)."""
    rng = np.random.default_rng(seed)
    n = len(G)
    G2 = G.copy()
    used = set(int(a) for a in anchors) | set(int(a) for a in avoid)
    rivals = np.empty(len(anchors), np.int64)
    for i, a in enumerate(anchors):
        r = (int(a) + n // 2) % n
        while r in used:
            r = (r + 1) % n
        used.add(r)
        rivals[i] = r
    g = G[anchors].copy()
    diff = np.abs(np.asarray(q, np.float32) - g)
    col = np.argmax(diff, axis=1)
    steps = rng.integers(1, 65, len(anchors)) * rng.choice([-1, 1], len(anchors))
    bits = g[np.arange(len(anchors)), col].view(np.int32).astype(np.int64) + steps
    g[np.arange(len(anchors)), col] = bits.astype(np.int32).view(np.float32)
    G2[rivals] = g
    return G2, rivals


# ---------------------------------------------------------------------------------------
# Ill-conditioned features (test_gpu_search_conditioning.py; conditions checked on the
# reference alone in test_parity_generators_cpu.py).  Each generator returns (gallery, probes)
# in fp32.
# ---------------------------------------------------------------------------------------
def offset_cluster(n, b, k, c, seed):
    """N(0, 1) + c for gallery and probes: every row shares a large common offset, so the
    expanded form ||g||^2 - 2 q.g cancels ~ c^2 k against differences of ~ k and an fp32 scan
    score is mostly rounding noise (c = 1000) or partly so (c = 30)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, k), dtype=np.float32) + np.float32(c)
    q = rng.standard_normal((b, k), dtype=np.float32) + np.float32(c)
    return g, q


def norm_outlier(n, b, k, seed):
    """Unit-scale rows, rows 0 and n - 1 multiplied by 2^12; each probe is a gallery row of
    ordinary norm times 1 + 0.05 N(0, 1) per component.  max ||g||^2, which the error bound and
    the tie window's scale are built from, is 2^24 times the norms that matter."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, k), dtype=np.float32)
    g[0] *= np.float32(4096.0)
    g[n - 1] *= np.float32(4096.0)
    src = rng.integers(1, n - 1, b)
    q = g[src] * (np.float32(1.0) + np.float32(0.05) * rng.standard_normal((b, k), dtype=np.float32))
    return g, q.astype(np.float32)


def dominant_component(n, b, k, seed):
    """N(0, 1) with column 0 multiplied by 1000: the first principal component dwarfs the rest
    (features of an unwhitened PCA)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, k), dtype=np.float32)
    q = rng.standard_normal((b, k), dtype=np.float32)
    g[:, 0] *= np.float32(1000.0)
    q[:, 0] *= np.float32(1000.0)
    return g, q


CONDITIONING_KS = (13, 128, 200, 600)  # padded 16 / 128 / 256 / 640
CONDITIONING_GENERATORS = ("offset30", "offset1000", "norm_outlier", "dominant")
MIN_CLEAR = 0.95  # share of probes the fp64 reference alone must leave outside the tie window


def conditioning_shapes(k):
    """(n, b) used at feature width k."""
    return ((193, 257), (3001, 300)) if k in (128, 600) else ((193, 257),)


def conditioning_case(name, n, b, k):
    seed = 9000 + 7 * k + n
    if name == "offset30":
        return offset_cluster(n, b, k, 30.0, seed)
    if name == "offset1000":
        return offset_cluster(n, b, k, 1000.0, seed)
    if name == "norm_outlier":
        return norm_outlier(n, b, k, seed)
    if name == "dominant":
        return dominant_component(n, b, k, seed)
    raise ValueError(name)


def fp32_expanded_argmin(q, g):
    """What a plain fp32 scan of the expanded form returns: argmin of fp32(||g||^2) -
    2 fp32(q @ g.T), every operation in fp32."""
    q32, g32 = np.asarray(q, np.float32), np.asarray(g, np.float32)
    gn = (g32 * g32).sum(1, dtype=np.float32)
    return np.argmin(gn[None, :] - np.float32(2.0) * (q32 @ g32.T), axis=1)


def l2_scores_diff(q, g, idx):
    """fp64 squared distance in difference form of probe p to row idx[p]."""
    d = np.asarray(q, np.float64) - np.asarray(g, np.float64)[np.asarray(idx)]
    return (d * d).sum(1)


# ---------------------------------------------------------------------------------------
# Identity with the fp64 pipeline (test_gpu_pipeline_identity.py): pixels in, index out.
#
# Reference: orc.project in fp64 for gallery and probes, then the fp64 ranking of top2 on those
# features.  Engine: its own projection kernel for both (Engine.project for the gallery,
# Engine.recognize for the probes), then its search, which is exact on its own features up to
# the tie window.  The two can differ only through the projection's error, which
# test_gpu_project.py bounds per coordinate j of the features f' of an image p:
#   fp32 (test_project_u8):              |f'_j - f_j| <= 2e-6 sum_px |p - mu| |w_j| + 1e-6
#   bf16 (test_project_bf16_tolerance):  |f'_j - f_j| <= 2^-8 sum_px |p - rint(mu)| |w_j|
#                                                        + 2e-6 sum_px |p - mu| |w_j| + 1e-5
# (mu in 0..255, so |p - rint(mu)| <= 256 is exact in bf16: one rounding).  eps(p) is the 2-norm
# of that bound vector, so ||f' - f|| <= eps(p).
#
# L2, in distances (not squared).  With d(p, r) = ||f_p - g_r|| and d' the same on the engine's
# features, the triangle inequality gives |d' - d| <= eps(p) + eps(r) <= E_p = eps(p) + max_r
# eps(r).  Let r* be the fp64 best with distance d1 and every other row at d >= d2.  If
# d2 - d1 > 2 E_p + sqrt(W), then d'(r) - d'(r*) > sqrt(W) for every other r, hence
# d'(r)^2 > d'(r*)^2 + W: r* is the engine's arg-min outside a window W on the squared distances.
# W = MARGIN * 1e-12 ((d1 + E_p)^2 + (||f_p|| + eps(p))^2 + (max ||g_r|| + max eps(r))^2) is an
# upper bound of the engine's tie window on its own features.  Conversely the engine's row r'
# has d'(r')^2 <= d'(r*)^2 + W, so d'(r') <= d'(r*) + sqrt(W) and d(r') <= d1 + 2 E_p + sqrt(W).
#
# Cosine, in chord lengths c(p, r) = ||f_p/||f_p|| - g_r/||g_r|| || = sqrt(2 (1 + s)), s = -cos the
# engine's score (same order).  ||x'/||x'|| - x/||x|| || <= 2 ||x' - x|| / ||x||, so
# |c' - c| <= H_p = 2 eps(p)/||f_p|| + max_r 2 eps(r)/||g_r||, and the same argument holds with
# (c, H_p) in place of (d, E_p) and Wc = 2 * MARGIN * 1e-12 * 2 (the window 1e-12 (|s| + 1) <= 2e-12
# on s is twice that on c^2 = 2 (1 + s)).
# ---------------------------------------------------------------------------------------
PIPELINE_D, PIPELINE_N, PIPELINE_NEAR, PIPELINE_MID = 4096, 2000, 100, 200
PIPELINE_CASES = ((64, "fp32"), (512, "fp32"), (512, "bf16"))


# The fp64 top-2 margins the midpoint probes are steered to, per metric (L2 distances, cosine
# chord lengths): geometric sweeps from well under the case's identity bound to well over it.
# The bounds (test_parity_generators_cpu.py prints them): L2 ~ 0.2 (k = 64) and 0.6 (k = 512) in
# fp32, ~ 1.2e3 in bf16, where a full move to one image gives ~ 2.4e3; cosine ~ 8e-4 in fp32.
# The bf16 cosine bound, ~ 1.4, exceeds every chord margin there is (sqrt(2) for an exact copy of
# a gallery image among unrelated ones): that case guarantees no identity and only (b) applies.
PIPELINE_MARGINS = {
    (64, "fp32"): {"l2": (0.004, 6.0), "cosine": (1.6e-5, 0.025)},
    (512, "fp32"): {"l2": (0.012, 18.0), "cosine": (1.5e-5, 0.022)},
    (512, "bf16"): {"l2": (300.0, 20000.0), "cosine": (1e-3, 1.0)},
}


def _steer_to_margin(x, a, gain, target, tol, order):
    """Move pixels of x (in place) to a's values, in the seeded order `order`, each only when it
    brings the margin's first-order estimate (sum of the moved pixels' gains) closer to the
    target; stops within tol of it."""
    m = 0.0
    for i in order:
        if abs(m - target) <= tol:
            break
        if abs(m + gain[i] - target) < abs(m - target):
            m += gain[i]
            x[i] = a[i]


def pipeline_case(k, precision):
    """(mean fp32 (d,), W fp32 (d, k) orthonormal columns, gallery uint8 (n, d), probes uint8
    (b, d)): 100 probes are gallery images plus noise in -3..3; 200 start at the pixel midpoint x
    of two gallery images a and c and are moved to a's values on a subset of pixels, taken in a
    seeded random order, that steers the fp64 margin m(x) = dist(x, c) - dist(x, a) to the probe's
    entry of the sweep PIPELINE_MARGINS: even probes the L2 distance, odd ones the cosine chord.
    A pixel is moved when that brings the first-order estimate of m closer to the target.  With
    f = (x - mean) W and a pixel i changed by t, f changes by t w_i, and
      L2:     grad_f m = 2 u, u the unit vector from c's features to a's (both distances ~ D/2);
      cosine: grad_f m = P (a^/c_a - c^/c_c) / ||f||, P = I - f^ f^T, r^ unit features, c_r the chords."""
    rng = np.random.default_rng(4000 + k)
    d, n = PIPELINE_D, PIPELINE_N
    mean = rng.uniform(60, 200, d).astype(np.float32)
    w = np.linalg.qr(rng.standard_normal((d, k)))[0].astype(np.float32)
    gal = rng.integers(0, 256, (n, d), dtype=np.uint8)
    near = np.clip(gal[:PIPELINE_NEAR].astype(np.int32) + rng.integers(-3, 4, (PIPELINE_NEAR, d)), 0, 255)
    pair = rng.permutation(n)[:2 * PIPELINE_MID].reshape(PIPELINE_MID, 2)
    a, c = gal[pair[:, 0]].astype(np.int32), gal[pair[:, 1]].astype(np.int32)
    mid = (a + c) // 2
    w64, mu = w.astype(np.float64), mean.astype(np.float64)
    fa, fc, fx = (a - mu) @ w64, (c - mu) @ w64, (mid - mu) @ w64
    sweep = PIPELINE_MARGINS[(k, precision)]
    targets = {m: np.geomspace(*sweep[m], PIPELINE_MID // 2) for m in sweep}
    srng = np.random.default_rng(5000 + k + (1 if precision == "bf16" else 0))
    for i in range(PIPELINE_MID):
        if i % 2 == 0:
            grad = 2.0 * (fa[i] - fc[i]) / np.linalg.norm(fa[i] - fc[i])
            start = np.linalg.norm(fx[i] - fc[i]) - np.linalg.norm(fx[i] - fa[i])
            target = targets["l2"][i // 2]
        else:
            ua, uc, ux = (v / np.linalg.norm(v) for v in (fa[i], fc[i], fx[i]))
            ca, cc = np.linalg.norm(ux - ua), np.linalg.norm(ux - uc)
            grad = ua / ca - uc / cc
            grad = (grad - ux * (ux @ grad)) / np.linalg.norm(fx[i])
            start = cc - ca
            target = targets["cosine"][i // 2]
        gain = (a[i] - mid[i]) * (w64 @ grad)
        _steer_to_margin(mid[i], a[i], gain.tolist(), float(target - start), 0.02 * float(target),
                         srng.permutation(d).tolist())
    probes = np.concatenate([near, mid]).astype(np.uint8)
    return mean, w, gal, probes


def projection_eps(p, mean, w, precision):
    """eps(p): the 2-norm over the k coordinates of the projection's tested error bound."""
    p64, mu, aw = np.asarray(p, np.float64), np.asarray(mean, np.float64), np.abs(np.asarray(w, np.float64))
    fp32 = 2e-6 * (np.abs(p64 - mu) @ aw)
    if precision == "bf16":
        bound = 2.0 ** -8 * (np.abs(p64 - np.rint(mu)) @ aw) + fp32 + 1e-5
    else:
        bound = fp32 + 1e-6
    return np.sqrt((bound ** 2).sum(1))


class PipelineReference:
    """The fp64 pipeline on one case and the per-probe bound under which the engine's row must
    be its row (derivation above).  Distances are L2 distances or cosine chord lengths."""

    def __init__(self, mean, w, gal, probes, precision):
        self.f = orc.project(probes, mean, w)
        self.g = orc.project(gal, mean, w)
        self.eps_p = projection_eps(probes, mean, w, precision)
        self.eps_g = projection_eps(gal, mean, w, precision)
        self.fn = np.linalg.norm(self.f, axis=1)
        self.gn = np.linalg.norm(self.g, axis=1)

    def distances(self, metric):
        """(b, n) fp64 distances of the reference pipeline."""
        if metric == "l2":
            d2 = (self.fn ** 2)[:, None] + (self.gn ** 2)[None, :] - 2.0 * (self.f @ self.g.T)
            return np.sqrt(np.maximum(d2, 0.0))
        s = -(orc._unit_rows(self.f) @ orc._unit_rows(self.g).T)
        return np.sqrt(np.maximum(2.0 * (1.0 + s), 0.0))

    def bound(self, metric, d1):
        """Per probe: the top-2 margin above which identity is guaranteed; also the distance
        excess the engine's row may have otherwise."""
        if metric == "l2":
            e = self.eps_p + self.eps_g.max()
            w = MARGIN * WINDOW * ((d1 + e) ** 2 + (self.fn + self.eps_p) ** 2 + (self.gn.max() + self.eps_g.max()) ** 2)
        else:
            e = 2.0 * self.eps_p / self.fn + (2.0 * self.eps_g / self.gn).max()
            w = 4.0 * MARGIN * WINDOW
        return 2.0 * e + np.sqrt(w)

    def margins(self, metric):
        """(first-best row, its distance, top-2 margin, bound, distances) per probe."""
        dist = self.distances(metric)
        idx = np.argmin(dist, axis=1)
        rows = np.arange(len(dist))
        d1 = dist[rows, idx]
        rest = dist.copy()
        rest[rows, idx] = np.inf
        return idx, d1, rest.min(axis=1) - d1, self.bound(metric, d1), dist


def assert_pipeline_identity(ref, metric, got_idx, min_guaranteed=None):
    """(a) the engine's row is the fp64 pipeline's wherever the fp64 margin exceeds the bound;
    (b) elsewhere its fp64-pipeline distance is within the bound of the best."""
    idx, d1, margin, bound, dist = ref.margins(metric)
    got = np.asarray(got_idx)
    assert ((got >= 0) & (got < dist.shape[1])).all()
    sure = margin > bound
    miss = sure & (got != idx)
    assert not miss.any(), f"{metric}: {miss.sum()} of {sure.sum()} probes with a margin above the bound differ " \
                           f"from the fp64 pipeline (first {np.flatnonzero(miss)[:5]})"
    mine = dist[np.arange(len(got)), got]
    far = ~(mine - d1 <= bound)
    assert not far.any(), f"{metric}: {far.sum()} probes chose a row farther than the bound from the fp64 best " \
                          f"(first {np.flatnonzero(far)[:5]})"
    if min_guaranteed is not None:
        assert sure.sum() >= min_guaranteed, sure.sum()
    return sure
