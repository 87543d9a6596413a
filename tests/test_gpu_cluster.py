"""Gallery clustering (ef_gallery_cluster) against the numpy reference of cluster_util: labels,
degree and info[0:3] as exact integer arrays.  Every generator asserts its own conditions on the
fp64 reference before the GPU is asked; delta comes from the formula in include/eigenface.h, never
from the kernel's output."""
import functools

import numpy as np
import pytest

import cluster_util as cu
from eigenface import _native as N

pytestmark = pytest.mark.gpu


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _run(eng, g, metric, t, min_samples=1):
    eng.set_gallery(g)
    lab, deg, info = eng.cluster_gallery(t, metric, min_samples, degree=True)
    assert lab.dtype == np.int32 and deg.dtype == np.int32 and info.dtype == np.int64
    assert lab.shape == deg.shape == (g.shape[0],) and info.shape == (4,)
    return lab, deg, info


def _check(got, ref):
    lab, deg, info = got
    rlab, rdeg, rinfo = ref
    np.testing.assert_array_equal(deg, rdeg)
    np.testing.assert_array_equal(lab, rlab)
    np.testing.assert_array_equal(info[:3], rinfo)
    assert info[3] >= 0 and not info[3] & N.EF_CLUSTER_UNCONVERGED


def _no_score_at(s, t):
    """An input condition: no pair so close to t that two fp64 formulas could disagree."""
    v = cu.upper(s)
    assert (np.abs(v - t) > 1e-12 * max(abs(t), 1e-300)).all()


# ------------------------------------------------------------------ blob galleries
BLOBS = ((129, 8), (300, 100), (700, 130), (513, 640))


@functools.lru_cache(maxsize=None)
def blob_case(n, k, metric):
    # seed 22: at (129, 8) two of the five classes lie within t of each other and merge
    g, cls = cu.blobs(n, k, 5, 22 if (n, k) == (129, 8) else 100 * n + k)
    s = cu.pair_scores(g, metric)
    t, half = cu.widest_gap(s, 3.0 * k, 5.0 * k) if metric == "l2" else cu.widest_gap(s, 0.3, 0.9)
    d = cu.delta(g, metric, s)
    assert half > d, (half, d)  # the threshold's gap is wider than the scan's error
    ref = cu.reference(g, metric, t, 1, s)
    assert 1 < ref[2][0] < n and ref[2][2] > 0
    if (n, k) == (129, 8):  # the topology is not the class partition
        from eigenface import pair_confusion
        tp, fp, fn, tn = pair_confusion(cls, ref[0])
        assert fp > 0 and ref[2][0] < 5
    _freeze(g, *ref)
    return g, t, ref


@pytest.mark.parametrize("metric", ("l2", "cosine"))
@pytest.mark.parametrize("n,k", BLOBS)
def test_blobs(eng, n, k, metric):
    g, t, ref = blob_case(n, k, metric)
    _check(_run(eng, g, metric, t), ref)


# ------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("metric", ("l2", "cosine"))
@pytest.mark.parametrize("n", (1, 2, 127, 128, 129, 257))
def test_tile_edges(eng, n, metric):
    """Every row identical except the last: the clamped re-reads of the last row past n (in the
    row tile and in the probe tile) link nothing, not even the last row with itself."""
    rng = np.random.default_rng(n)
    g = np.tile(rng.standard_normal(24).astype(np.float32), (n, 1))
    g[-1] = -g[0]
    t = 1.0 if metric == "l2" else 0.5
    ref = cu.reference(g, metric, t)
    assert ref[2][0] == min(n, 2) and ref[1][-1] == 0 and (ref[1][:-1] == n - 2).all()
    _check(_run(eng, g, metric, t), ref)


# ------------------------------------------------------------------ a path
def test_path_is_one_component(eng):
    n = 700
    rng = np.random.default_rng(5)
    g = np.zeros((n, 16), np.float32)
    g[:, 3] = rng.permutation(n)  # unit steps on a line; only neighbours are within t
    t = 2.25
    ref = cu.reference(g, "l2", t)
    assert ref[2][0] == 1 and ref[2][2] == n - 1 and ref[1].max() == 2
    _check(_run(eng, g, "l2", t), ref)


# ------------------------------------------------------------------ integer features
@functools.lru_cache(maxsize=None)
def integer_case(n, k):
    rng = np.random.default_rng(n + k)
    centres = rng.integers(-7, 8, (6, k))
    g = np.clip(centres[rng.integers(0, 6, n)] + rng.integers(-1, 2, (n, k)), -8, 8).astype(np.float32)
    s = cu.pair_scores(g, "l2")
    assert (s == np.rint(s)).all() and s.max() < 2 ** 23  # every fp32 partial sum is an exact integer
    v = cu.upper(s)
    w = v[v < 3 * k]
    t = float(w[w.size // 2])
    assert (v == t).any() and (v == t + 1).any() and (v == t - 1).any()
    _freeze(g)
    return g, s, t


@pytest.mark.parametrize("n,k", ((300, 20), (200, 130)))
def test_integer_scores_hit_the_threshold(eng, n, k):
    """A score equal to t links; t + 1 does not."""
    g, s, t = integer_case(n, k)
    at, below = cu.reference(g, "l2", t, 1, s), cu.reference(g, "l2", t - 1, 1, s)
    assert at[2][2] > below[2][2] > 0
    _check(_run(eng, g, "l2", t), at)
    _check(_run(eng, g, "l2", t - 1), below)


# ------------------------------------------------------------------ exact duplicates at t = 0
def test_exact_duplicates(eng):
    rng = np.random.default_rng(11)
    g = rng.standard_normal((200, 50)).astype(np.float32)
    g[10] = g[3]
    g[150] = g[3]
    g[77] = g[20]
    g[90] = g[40]
    g[90, 7] = np.nextafter(g[40, 7], np.float32(np.inf))  # one fp32 ulp apart in one component
    ref = cu.reference(g, "l2", 0.0)
    assert ref[2][2] == 4 and ref[2][0] == 197 and ref[0][90] != ref[0][40]
    assert ref[0][10] == ref[0][150] == ref[0][3] and ref[0][77] == ref[0][20]
    _check(_run(eng, g, "l2", 0.0), ref)


# ------------------------------------------------------------------ the band
@functools.lru_cache(maxsize=None)
def band_case():
    rng = np.random.default_rng(3)
    g = (3.0 * rng.standard_normal((64, 100))).astype(np.float32)
    pairs = [(2 * p, 2 * p + 33) for p in range(8)]
    for p, (a, b) in enumerate(pairs):
        # squared distance 4 (1 + tau), tau = -1.05e-7 .. 1.05e-7 in steps of 3e-8: a step of
        # 2 - 2^-22 in one component (an fp32 ulp is too coarse alone) and a small one in another
        c, c2 = 5 + 11 * p, 6 + 11 * p
        g[a, c], g[a, c2] = 1.0, 0.0
        g[b] = g[a]
        g[b, c] = np.nextafter(np.float32(3.0), np.float32(0.0))
        step = float(g[b, c]) - 1.0
        g[b, c2] = np.float32(np.sqrt(4.0 * (1.0 + (p - 3.5) * 3e-8) - step * step))
    s = cu.pair_scores(g, "l2")
    planted = np.array([s[a, b] for a, b in pairs])
    order = np.sort(planted)
    assert (np.diff(order) > 1.3e-8 * 4).all() and abs(order[0] - 4) < 1e-6 and abs(order[7] - 4) < 1e-6
    t = 0.5 * (order[3] + order[4])
    d = cu.delta(g, "l2", s)
    assert (np.abs(planted - t) < d).all()  # all eight are inside the band
    _no_score_at(s, t)
    v = cu.upper(s)
    assert (v < 5).sum() == 8 and v[8] > 1000  # every other pair is far away
    ref = cu.reference(g, "l2", t, 1, s)
    assert ref[2][2] == 4 and ref[2][0] == 60
    _freeze(g, *ref)
    return g, t, ref


def test_band_is_settled_in_fp64(eng):
    g, t, ref = band_case()
    got = _run(eng, g, "l2", t)
    _check(got, ref)
    assert got[2][3] >= 8  # the pairs settled in fp64


# ------------------------------------------------------------------ density floor
@functools.lru_cache(maxsize=None)
def density_case():
    """Twice (at y = 0 and y = 30): two tight blobs 3.6 apart, each with an outpost 0.9 towards the
    other, and one border row midway that is within t = 1 of the two outposts only.  Then three
    isolated rows and a far pair linked only to each other.  Rows in random order."""
    rng = np.random.default_rng(17)
    k = 16

    def at(x, y, m):
        p = 0.02 * rng.standard_normal((m, k))
        p[:, 0] += x
        p[:, 1] += y
        return p
    rows = []
    for y in (0.0, 30.0):  # roles 0 .. 4 and 5 .. 9: blob, blob, outpost, outpost, border
        rows += [at(0.0, y, 30), at(3.6, y, 30), at(0.9, y, 1), at(2.7, y, 1), at(1.8, y, 1)]
    rows += [at(50.0, 0.0, 1), at(-60.0, 0.0, 1), at(80.0, 0.0, 1)]  # roles 10 .. 12: isolated
    rows += [at(20.0, 60.0, 2)]                                      # role 13: the far pair
    g = np.concatenate(rows)
    role = np.concatenate([np.full(r.shape[0], i) for i, r in enumerate(rows)])
    perm = rng.permutation(g.shape[0])
    g, role = g[perm].astype(np.float32), role[perm]
    s = cu.pair_scores(g, "l2")
    t = 1.0
    assert cu.widest_gap(s, 0.9, 1.1)[1] > 10 * cu.delta(g, "l2", s)
    refs = {ms: cu.reference(g, "l2", t, ms, s) for ms in (1, 2, 4)}
    border = np.flatnonzero((role == 4) | (role == 9))
    deg = refs[1][1]
    assert (deg[border] == 2).all() and (deg[role == 13] == 1).all() and (deg[(role >= 10) & (role <= 12)] == 0).all()
    # min_samples = 2: the border rows are core and merge their two blobs; the pair is a cluster;
    # the isolated rows are noise
    assert refs[2][2][0] == 3 and refs[2][2][1] == 3
    # min_samples = 4: a border row is not core and takes the cluster of its lowest-index outpost;
    # the blobs stay apart; the pair is noise too
    lab4 = refs[4][0]
    assert refs[4][2][0] == 4 and refs[4][2][1] == 5
    for r, (ra, rb) in ((4, (2, 3)), (9, (7, 8))):
        row = np.flatnonzero(role == r)[0]
        a_out, b_out = np.flatnonzero(role == ra)[0], np.flatnonzero(role == rb)[0]
        assert lab4[a_out] != lab4[b_out] and lab4[row] == lab4[min(a_out, b_out)]
    _freeze(g)
    return g, t, refs


@pytest.mark.parametrize("min_samples", (1, 2, 4))
def test_density_floor(eng, min_samples):
    g, t, refs = density_case()
    _check(_run(eng, g, "l2", t, min_samples), refs[min_samples])


# ------------------------------------------------------------------ non-finite and zero rows
@pytest.mark.parametrize("min_samples", (1, 2))
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_non_finite_rows(eng, metric, min_samples):
    g, _ = cu.blobs(200, 24, 4, 99)
    g = g.copy()
    clean = cu.pair_scores(g, metric)
    t, half = cu.widest_gap(clean, 72, 120) if metric == "l2" else cu.widest_gap(clean, 0.3, 0.9)
    assert half > cu.delta(g, metric, clean)
    g[5, 3] = np.nan
    g[77, 0] = np.inf
    g[130, 23] = -np.inf
    bad = np.array([5, 77, 130])
    ref = cu.reference(g, metric, t, min_samples)
    base = cu.reference(np.delete(g, bad, axis=0), metric, t, min_samples)
    assert (ref[1][bad] == 0).all()
    if min_samples > 1:
        assert (ref[0][bad] == -1).all()
    else:
        assert np.unique(ref[0][bad]).size == 3 and all((ref[0] == ref[0][b]).sum() == 1 for b in bad)
    np.testing.assert_array_equal(np.delete(ref[1], bad), base[1])  # the other rows are unaffected
    _check(_run(eng, g, metric, t, min_samples), ref)


@pytest.mark.parametrize("t", (1e-3, 0.0, -1e-3))
def test_zero_rows_under_cosine(eng, t):
    """A zero row scores 0 against every row: unlinked above t = 0, linked to all at and below."""
    rng = np.random.default_rng(23)
    g = rng.standard_normal((150, 40)).astype(np.float32)
    zero = np.array([0, 70, 149])
    g[zero] = 0.0
    s = cu.pair_scores(g, "cosine")
    assert (s[zero] == 0.0).all()
    nz = np.delete(np.arange(150), zero)
    assert (np.abs(cu.upper(s[np.ix_(nz, nz)]) - t) > 1e-9).all()
    ref = cu.reference(g, "cosine", t, 1, s)
    assert (ref[1][zero] == (0 if t > 0 else 149)).all()
    _check(_run(eng, g, "cosine", t), ref)


# ------------------------------------------------------------------ device tensors, determinism
def test_device_tensors_on_a_callers_stream(eng):
    import torch
    g, t, ref = blob_case(700, 130, "l2")
    eng.set_gallery(g)
    n = g.shape[0]
    stream = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(stream):
        for _ in range(2):
            lab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            deg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            l2, d2, info = eng.cluster_gallery(t, "l2", 1, degree=deg, labels=lab)
            assert l2 is lab and d2 is deg and info.is_cuda and info.dtype == torch.int64
            outs.append((lab, deg, info))
    stream.synchronize()
    a, b = ([x.cpu().numpy() for x in o] for o in outs)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)  # bit-identical
    _check(a, ref)
    # labels alone: no degree comes back
    with torch.cuda.stream(stream):
        lab = torch.empty(n, dtype=torch.int32, device="cuda")
        _, none, info = eng.cluster_gallery(t, "l2", labels=lab)
    stream.synchronize()
    assert none is None
    np.testing.assert_array_equal(lab.cpu().numpy(), ref[0])


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_all_rows_identical(eng, metric):
    n = 4096
    g = np.tile(np.random.default_rng(1).standard_normal(128).astype(np.float32), (n, 1))
    outs = [_run(eng, g, metric, 0.5) for _ in range(2)]
    for lab, deg, info in outs:
        assert (lab == 0).all() and (deg == n - 1).all()
        assert info[0] == 1 and info[1] == 0 and info[2] == n * (n - 1) // 2
        assert not info[3] & N.EF_CLUSTER_UNCONVERGED
    np.testing.assert_array_equal(outs[0][2], outs[1][2])


# ------------------------------------------------------------------ state and arguments
def test_state_and_arguments(eng):
    import torch
    from eigenface import Engine
    lib = N.lib()
    lab = np.zeros(8, np.int32)
    info = np.zeros(4, np.int64)
    with Engine(0) as fresh:
        with pytest.raises(RuntimeError):
            fresh.cluster_gallery(1.0)
        rc = lib.ef_gallery_cluster(fresh._h, N.EF_METRIC_L2, 1.0, 1, lab.ctypes.data, None, info.ctypes.data, 0)
        assert rc == N.EF_E_STATE
    g = np.random.default_rng(2).standard_normal((8, 5)).astype(np.float32)
    eng.set_gallery(g)
    with pytest.raises(ValueError):
        eng.cluster_gallery(float("nan"))
    args = (lab.ctypes.data, None, info.ctypes.data, 0)
    assert lib.ef_gallery_cluster(eng._h, N.EF_METRIC_L2, float("nan"), 1, *args) == N.EF_E_INVALID
    assert lib.ef_gallery_cluster(eng._h, 7, 1.0, 1, *args) == N.EF_E_INVALID
    assert lib.ef_gallery_cluster(eng._h, N.EF_METRIC_L2, 1.0, 1, None, None, info.ctypes.data, 0) == N.EF_E_INVALID
    assert lib.ef_gallery_cluster(eng._h, N.EF_METRIC_L2, 1.0, 1, lab.ctypes.data, None, None, 0) == N.EF_E_INVALID
    assert lib.ef_gallery_cluster(eng._h, N.EF_METRIC_L2, 1.0, 1, *args) == N.EF_OK
    for bad in (torch.zeros(9, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda"),
                torch.zeros((8, 1), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            eng.cluster_gallery(1.0, labels=bad)
    with pytest.raises(TypeError):
        eng.cluster_gallery(1.0, labels=np.zeros(8, np.int32))
    # new rows: the next call clusters them, not the old gallery
    g1, t1, ref1 = blob_case(129, 8, "l2")
    _check(_run(eng, g1, "l2", t1), ref1)
    g2, t2, ref2 = blob_case(300, 100, "l2")
    _check(_run(eng, g2, "l2", t2), ref2)


def test_result_object(eng):
    from eigenface import cluster_gallery
    g, t, refs = density_case()
    eng.set_gallery(g)
    r = cluster_gallery(eng, t, "l2", min_samples=4, degree=True)
    lab = refs[4][0]
    np.testing.assert_array_equal(r.labels, lab)
    assert r.n_clusters == refs[4][2][0] and r.n_noise == refs[4][2][1] and r.n_links == refs[4][2][2]
    np.testing.assert_array_equal(r.sizes, np.bincount(lab[lab >= 0]))
    np.testing.assert_array_equal(r.representatives, [np.flatnonzero(lab == c)[0] for c in range(r.n_clusters)])
    np.testing.assert_array_equal(r.degree, refs[4][1])


# ------------------------------------------------------------------ one larger case
def test_larger_gallery(eng):
    n, k = 8192, 128
    g, cls = cu.blobs(n, k, 64, 4242)
    s = cu.pair_scores(g, "l2", gram=True)
    t, half = cu.widest_gap(s, 3.0 * k, 5.0 * k)
    # the gram form's own error is far below the gap: 1e-9 covers it with room
    assert half > cu.delta(g, "l2", s) + 1e-9 * s.max()
    ref = cu.reference(g, "l2", t, 1, s)
    assert ref[2][0] == 64
    _check(_run(eng, g, "l2", t), ref)


# ------------------------------------------------------------------ work items of several tiles
# Below n = 11521 every link item is one row tile, and below n = 65537 the label scan is one
# round.  The lattice of cluster_util has its exact answer from a dict of points in O(n k), so
# the sizes past those lines need no n x n reference.
LINE = 65536  # rows in one round of cluster_scan_kernel: 256 blocks of 256


def _plan(n):
    """(row tiles, tiles per link item, tiles per count item): cluster_tiles_per_item restated."""
    tiles = (n + 127) // 128
    return tiles, min(tiles, max(1, tiles * (tiles + 1) // 2 // 2048)), min(tiles, max(1, tiles * tiles // 2048))


def _differs_from_tile_to_tile(x):
    """An input condition: a per-row value taken from the tile before or after is another value."""
    assert (x[:-128] != x[128:]).mean() > 0.9


def _run_device(eng, t, metric, min_samples, n):
    """The device-tensor form on the resident gallery, as host arrays."""
    import torch
    lab = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    deg = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    l2, d2, info = eng.cluster_gallery(t, metric, min_samples, degree=deg, labels=lab)
    assert l2 is lab and d2 is deg and info.is_cuda and info.dtype == torch.int64
    return tuple(x.cpu().numpy() for x in (lab, deg, info))


@functools.lru_cache(maxsize=None)
def lattice_case(n, k):
    g = cu.lattice(n, k, n + k)
    if n > LINE:
        # three whole clusters of the min_samples = 4 reference go behind the line, so that
        # their roots lie there at every min_samples
        lab = cu.lattice_reference(g, 4)[0]
        sizes = np.bincount(lab[lab >= 0])
        rows = np.flatnonzero(np.isin(lab, np.flatnonzero((sizes >= 4) & (sizes <= 8))[-3:]))
        tail = np.arange(n - rows.size, n)
        src, dst = np.setdiff1d(rows, tail), np.setdiff1d(tail, rows)
        g[np.concatenate([src, dst])] = g[np.concatenate([dst, src])]
    # scores 0 and 2 are decided by the fp32 scan, score 1 = t lies inside the band
    assert cu.delta(g, "l2", from_norms=True) < 0.5
    _differs_from_tile_to_tile((g.astype(np.float64) ** 2).sum(axis=1))
    _freeze(g)
    return g


@functools.lru_cache(maxsize=None)
def lattice_ref(n, k, min_samples, unit_steps=True):
    ref = cu.lattice_reference(lattice_case(n, k), min_samples, unit_steps)
    lab, deg, info = ref
    assert 1 < info[0] < n and info[2] > n // 8 and (np.bincount(lab[lab >= 0]) > 1).any()
    if min_samples > 1:
        core = deg + 1 >= min_samples
        assert info[1] > 0 and (~core).any() and core.any()
        assert (~core & (lab >= 0)).any() or not unit_steps  # rows attached to a core row of another point
    _freeze(*ref)
    return ref


@pytest.mark.parametrize("min_samples", (1, 4))
@pytest.mark.parametrize("k", (16, 40))
def test_link_items_of_several_tiles(eng, k, min_samples):
    """n = 11530: 91 row tiles with 10 rows in the last.  The link pass takes two row tiles per
    item (the diagonal tile second in items with t0 > 0), the count pass four, its last item
    ending on the ragged tile.  k = 16 is one slice per tile, k = 40 (kp = 64) four."""
    n = 11530
    assert _plan(n) == (91, 2, 4) and n - 90 * 128 == 10 and cu.kp_of(k) // 16 == (1 if k == 16 else 4)
    g = lattice_case(n, k)
    ref = lattice_ref(n, k, min_samples)
    got = _run(eng, g, "l2", 1.0, min_samples)
    _check(got, ref)
    assert got[2][3] >= cu.lattice_unit_pairs(g)  # the pairs at t itself are settled in fp64
    dev = _run_device(eng, 1.0, "l2", min_samples, n)
    for x, y in zip(dev, got):
        assert x.tobytes() == y.tobytes()


@functools.lru_cache(maxsize=None)
def cosine_threshold(n, k):
    """Midway between 1 and the largest cosine of two rows that are not the same point: then
    exactly the duplicates link."""
    g = lattice_case(n, k)
    top = cu.max_cosine_between_points(g)
    half = 0.5 * (1.0 - top)
    assert half > 4 * cu.delta(g, "cosine"), (half, cu.delta(g, "cosine"))
    return 1.0 - half


@pytest.mark.parametrize("min_samples", (1, 2))
@pytest.mark.parametrize("k", (16, 40))
def test_link_items_of_several_tiles_cosine(eng, k, min_samples):
    """The same plan under cosine, where the rows' 1 / |g| are read from the aux slot in the
    epilogue: only rows at the same point link."""
    n = 11530
    assert _plan(n) == (91, 2, 4)
    g = lattice_case(n, k)
    with np.errstate(divide="raise"):
        _differs_from_tile_to_tile(1.0 / np.sqrt((g.astype(np.float64) ** 2).sum(axis=1)))
    t = cosine_threshold(n, k)
    ref = lattice_ref(n, k, min_samples, False)
    got = _run(eng, g, "cosine", t, min_samples)
    _check(got, ref)
    if k == 16:
        dev = _run_device(eng, t, "cosine", min_samples, n)
        for x, y in zip(dev, got):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("min_samples", (1, 4))
def test_label_scan_carries_past_256_blocks(eng, min_samples):
    """n = 65836: 258 blocks of 256 rows, so cluster_scan_kernel runs a second round on the
    running total of the first; 515 row tiles, 64 per link item and 129 per count item."""
    n, k = 65836, 16
    assert (n + 255) // 256 == 258 and _plan(n) == (515, 64, 129)
    g = lattice_case(n, k)
    ref = lattice_ref(n, k, min_samples)
    lab, deg, info = ref
    core = deg + 1 >= min_samples
    roots = np.full(info[0], n, np.int64)  # by cluster: its lowest core row
    np.minimum.at(roots, lab[core], np.flatnonzero(core))
    assert (np.diff(roots) > 0).all()  # numbered in the order of their roots
    assert 3 <= (roots >= LINE).sum() < info[0]  # roots whose number needs the carry
    behind = lab[LINE:]
    assert (roots[behind[behind >= 0]] < LINE).any() and (roots[behind[behind >= 0]] >= LINE).any()
    if min_samples > 1:
        assert (lab[:LINE] < 0).any() and (behind < 0).any()  # noise on both sides
    got = _run(eng, g, "l2", 1.0, min_samples)
    _check(got, ref)
    assert got[2][3] >= cu.lattice_unit_pairs(g)
