"""Range search (ef_search_range) against the numpy reference of range_util: lims, rows and
info[0] as exact integer arrays, scores within delta of the fp64 scores.  Every generator asserts
its own conditions on the fp64 reference before the GPU is asked; delta comes from the formula in
include/eigenface.h, never from the kernel's output."""
import functools

import numpy as np
import pytest

import cluster_util as cu
import range_util as ru
from eigenface import _native as N
from eigenface import neighbors as nb

pytestmark = pytest.mark.gpu


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _run(eng, g, q, metric, t, exclude=None, offset=0, **kw):
    eng.set_gallery(g, global_offset=offset)
    r = eng.search_range(q, t, metric, exclude, **kw)
    assert r.lims.dtype == np.int64 and r.rows.dtype == np.int64 and r.scores.dtype == np.float32
    assert r.info.dtype == np.int64 and r.lims.shape == (q.shape[0] + 1,) and r.info.shape == (4,)
    return r


def _check(r, ref, q=None, g=None, metric=None, t=None):
    """Exact lims, rows and totals; with q and g also every score within delta_p of its fp64 score
    and on the accepting side of fp32(t)."""
    lims, rows, scores = ref
    np.testing.assert_array_equal(r.lims, lims)
    np.testing.assert_array_equal(r.rows, rows)
    assert r.info[0] == lims[-1] and r.info[1] >= 0 and r.info[2] == 0 and r.info[3] == 0
    assert r.complete and r.scores.shape == rows.shape
    if q is not None:
        d = np.repeat(ru.delta(q, g, metric, t), np.diff(lims))
        err = np.abs(r.scores.astype(np.float64) - scores)
        assert (err <= d).all(), float((err - d).max())
        t32 = np.float32(t)
        assert (r.scores <= t32).all() if metric == "l2" else (r.scores >= t32).all()


# ------------------------------------------------------------------ blob galleries
BLOBS = ((129, 8), (300, 100), (700, 130), (513, 640))


@functools.lru_cache(maxsize=None)
def blob_case(n, k, metric):
    g, _ = cu.blobs(n, k, 5, 100 * n + k)
    rng = np.random.default_rng(n + k)
    q = (g[rng.integers(0, n, 77)] + 0.3 * rng.standard_normal((77, k))).astype(np.float32)
    v = ru.finite_scores(q, g, metric)
    t, half = ru.widest_gap(v, 3.0 * k, 5.0 * k) if metric == "l2" else ru.widest_gap(v, 0.3, 0.9)
    assert half > ru.delta(q, g, metric, t).max()  # the threshold's gap is wider than the scan's error
    ref = ru.reference(q, g, metric, t)
    counts = np.diff(ref[0])
    assert counts.min() >= 1 and counts.max() < n and np.unique(counts).size > 1
    _freeze(g, q, *ref)
    return g, q, t, ref


@pytest.mark.parametrize("metric", ("l2", "cosine"))
@pytest.mark.parametrize("n,k", BLOBS)
def test_blobs(eng, n, k, metric):
    g, q, t, ref = blob_case(n, k, metric)
    _check(_run(eng, g, q, metric, t), ref, q, g, metric, t)


# ------------------------------------------------------------------ tile edges
@pytest.mark.parametrize("metric", ("l2", "cosine"))
@pytest.mark.parametrize("b", (1, 31, 33, 128, 129))
@pytest.mark.parametrize("n", (1, 2, 127, 128, 129, 257))
def test_tile_edges(eng, n, b, metric):
    """Every row identical except the last, every probe identical except the last: the clamped
    re-reads of the last row past n and the zero probes past b hit nothing."""
    v = np.random.default_rng(n).standard_normal(24).astype(np.float32)
    g = np.tile(v, (n, 1))
    g[-1] = -v
    q = np.tile(v, (b, 1))
    q[-1] = -v
    t = 1.0 if metric == "l2" else 0.5
    ref = ru.reference(q, g, metric, t)
    counts = np.diff(ref[0])
    assert counts[-1] == 1 and ref[1][-1] == n - 1 and (counts[:-1] == n - 1).all()
    _check(_run(eng, g, q, metric, t), ref)


# ------------------------------------------------------------------ integer features
@functools.lru_cache(maxsize=None)
def integer_case(n, k):
    rng = np.random.default_rng(n + k)
    centres = rng.integers(-7, 8, (6, k))
    x = np.clip(centres[rng.integers(0, 6, n + 50)] + rng.integers(-1, 2, (n + 50, k)), -8, 8).astype(np.float32)
    g, q = x[:n], x[n:]
    v = ru.finite_scores(q, g, "l2")
    assert (v == np.rint(v)).all() and v.max() < 2 ** 23  # every fp32 partial sum is an exact integer
    w = v[v < 3 * k]
    t = float(w[w.size // 2])
    assert (v == t).any() and (v == t + 1).any() and (v == t - 1).any()
    _freeze(g, q)
    return g, q, t


@pytest.mark.parametrize("n,k", ((300, 20), (200, 130)))
def test_integer_scores_hit_the_threshold(eng, n, k):
    """A score equal to t is a hit; t + 1 is not."""
    g, q, t = integer_case(n, k)
    at, below = ru.reference(q, g, "l2", t), ru.reference(q, g, "l2", t - 1)
    assert at[0][-1] > below[0][-1] > 0
    r = _run(eng, g, q, "l2", t)
    _check(r, at, q, g, "l2", t)
    np.testing.assert_array_equal(r.scores, at[2].astype(np.float32))  # exact integers
    _check(_run(eng, g, q, "l2", t - 1), below, q, g, "l2", t - 1)


# ------------------------------------------------------------------ the band
@functools.lru_cache(maxsize=None)
def band_case(seed):
    """tests/test_gpu_cluster.py's band_case with the b rows as probes: eight planted pairs at
    squared distance 4 (1 + tau), |tau| <= 1.05e-7, four on each side of t."""
    rng = np.random.default_rng(seed)
    x = (3.0 * rng.standard_normal((64, 100))).astype(np.float32)
    pairs = [(2 * p, 2 * p + 33) for p in range(8)]
    for p, (a, b) in enumerate(pairs):
        c, c2 = 5 + 11 * p, 6 + 11 * p
        x[a, c], x[a, c2] = 1.0, 0.0
        x[b] = x[a]
        x[b, c] = np.nextafter(np.float32(3.0), np.float32(0.0))
        step = float(x[b, c]) - 1.0
        x[b, c2] = np.float32(np.sqrt(4.0 * (1.0 + (p - 3.5) * 3e-8) - step * step))
    probes = np.array([b for _, b in pairs])
    g, q = np.delete(x, probes, axis=0), x[probes]
    arow = np.array([a - (probes < a).sum() for a, _ in pairs])  # the a rows inside g
    s = ru.block_scores(q, g, "l2")
    planted = s[np.arange(8), arow]
    order = np.sort(planted)
    assert (np.diff(order) > 1.3e-8 * 4).all() and abs(order[0] - 4) < 1e-6 and abs(order[7] - 4) < 1e-6
    t = 0.5 * (order[3] + order[4])
    assert (np.abs(planted - t) < ru.delta(q, g, "l2", t)).all()  # all eight are inside the band
    v = np.sort(s.ravel())
    ru.no_score_at(v, t)
    assert (v < 5).sum() == 8 and v[8] > 1000  # every other pair is far away
    ref = ru.reference(q, g, "l2", t)
    assert ref[0][-1] == 4 and set(np.diff(ref[0])) == {0, 1}
    _freeze(g, q, *ref)
    return g, q, t, ref


@pytest.mark.parametrize("seed", (3, 4))
def test_band_is_settled_in_fp64(eng, seed):
    """An fp32-only decision gets the eight planted pairs right by chance with probability 2^-8;
    no kernel without the band passes both seeds."""
    g, q, t, ref = band_case(seed)
    r = _run(eng, g, q, "l2", t)
    _check(r, ref, q, g, "l2", t)
    assert r.info[1] >= 8  # the pairs settled in fp64
    assert (r.scores <= np.float32(t)).all() and r.scores.size == 4
    np.testing.assert_array_equal(r.scores, ref[2].astype(np.float32))  # (float) of the fp64 score


# ------------------------------------------------------------------ dense hits and ordering
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_dense_hits_are_in_row_order(eng, metric):
    """Every probe hits every row: 64 hits per lane and tile, the two lane halves interleaved."""
    n, b = 300, 70
    v = np.random.default_rng(1).standard_normal(128).astype(np.float32)
    g, q = np.tile(v, (n, 1)), np.tile(v, (b, 1))
    r = _run(eng, g, q, metric, 0.5)
    assert r.info[0] == n * b == 21000 and r.complete
    np.testing.assert_array_equal(r.lims, np.arange(b + 1) * n)
    np.testing.assert_array_equal(r.rows.reshape(b, n), np.tile(np.arange(n), (b, 1)))
    want = 0.0 if metric == "l2" else 1.0
    assert np.abs(r.scores - want).max() <= ru.delta(q, g, metric, 0.5).max()


# ------------------------------------------------------------------ exclusion
def test_exclusion_and_global_offset(eng):
    rng = np.random.default_rng(12)
    n, off = 300, 5000
    g = rng.standard_normal((n, 40)).astype(np.float32)
    g[200] = g[7]  # a duplicate: excluding row 7 leaves row 200
    src = np.array([7, 7, 200, 11, 12, 13, 299, 0, 150, 150])
    q = g[src]
    excl = np.array([off + 7, -1, off + 7, off + 11, 12, off + n, off + 299, -5, off + 150 + n, off + 149], np.int64)
    ref = ru.reference(q, g, "l2", 0.0, excl, offset=off)
    want = [[off + 200], [off + 7, off + 200], [off + 200], [], [off + 12], [off + 13], [], [off], [off + 150],
            [off + 150]]
    assert [list(ref[1][ref[0][p]:ref[0][p + 1]]) for p in range(10)] == want
    r = _run(eng, g, q, "l2", 0.0, excl, offset=off)
    _check(r, ref, q, g, "l2", 0.0)
    assert (r.scores == 0.0).all()
    # without exclusions every probe finds its own row again
    r = _run(eng, g, q, "l2", 0.0, None, offset=off)
    _check(r, ru.reference(q, g, "l2", 0.0, None, offset=off))
    eng.set_gallery(g)  # the offset does not outlive this test


# ------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_non_finite_rows_and_probes(eng, metric):
    g, q, t, clean = (x.copy() if isinstance(x, np.ndarray) else x for x in blob_case(300, 100, metric))
    clean = ru.reference(q, g, metric, t)
    bad_rows, bad_probes = np.array([5, 77, 130]), np.array([3, 40])
    assert np.isin(clean[1], bad_rows).any() and (np.diff(clean[0])[bad_probes] > 0).all()
    g[5, 3] = np.nan
    g[77, 0] = np.inf
    g[130, 99] = -np.inf
    q[3, 50] = np.nan
    q[40, 1] = np.inf
    ref = ru.reference(q, g, metric, t)
    counts = np.diff(ref[0])
    assert (counts[bad_probes] == 0).all() and not np.isin(ref[1], bad_rows).any()
    # the other probes are unaffected beyond losing the bad rows
    for p in (0, 10, 76):
        seg = clean[1][clean[0][p]:clean[0][p + 1]]
        np.testing.assert_array_equal(ref[1][ref[0][p]:ref[0][p + 1]], seg[~np.isin(seg, bad_rows)])
    _check(_run(eng, g, q, metric, t), ref)


# ------------------------------------------------------------------ capacity
def test_capacity_and_count_only(eng):
    g, q, t, ref = blob_case(700, 130, "l2")
    lims, rows, scores = ref
    total, b = int(lims[-1]), q.shape[0]
    cap = total // 2
    fit = int(lims[lims <= cap][-1])
    nfit = int((lims[1:] <= cap).sum())
    assert 0 < fit < cap and 0 < nfit < b  # cap falls inside a segment
    eng.set_gallery(g)
    lib = N.lib()
    out_l = np.full(b + 1, -7, np.int64)
    out_r = np.full(cap + 16, -7, np.int64)
    out_s = np.full(cap + 16, -7.0, np.float32)
    info = np.full(4, -7, np.int64)
    rc = lib.ef_search_range(eng._h, q.ctypes.data, b, N.EF_METRIC_L2, t, None, out_l.ctypes.data, out_r.ctypes.data,
                             out_s.ctypes.data, cap, info.ctypes.data, 0)
    assert rc == N.EF_OK
    np.testing.assert_array_equal(out_l, lims)  # exact whatever the capacity
    np.testing.assert_array_equal(out_r[:fit], rows[:fit])
    d = np.repeat(ru.delta(q, g, "l2", t), np.diff(lims))[:fit]
    assert (np.abs(out_s[:fit].astype(np.float64) - scores[:fit]) <= d).all()
    assert (out_r[fit:] == -7).all() and (out_s[fit:] == -7.0).all()  # nothing at or past cap, nor in the gap
    np.testing.assert_array_equal(info, [total, info[1], total - fit, 0])
    # the wrapper: an incomplete result, then the same on device tensors with a canary behind cap
    r = eng.search_range(q, t, "l2", max_results=cap)
    assert r.complete is False and r.capacity == cap and r.rows.shape == (fit,) and r.info[2] == total - fit
    np.testing.assert_array_equal(r.of(nfit - 1)[0], rows[lims[nfit - 1]:lims[nfit]])
    with pytest.raises(ValueError):
        r.of(nfit)
    import torch
    big_r = torch.full((cap + 16,), -7, dtype=torch.int64, device="cuda")
    big_s = torch.full((cap + 16,), -7.0, dtype=torch.float32, device="cuda")
    rd = eng.search_range(torch.as_tensor(q.copy(), device="cuda"), t, "l2", out=(big_r[:cap], big_s[:cap]))
    assert rd.complete is None and rd.on_device and rd.capacity == cap
    torch.cuda.synchronize()
    assert big_r.cpu().numpy().tobytes() == out_r.tobytes() and big_s.cpu().numpy().tobytes() == out_s.tobytes()
    assert rd.host().complete is False and rd.host().rows.shape == (fit,)
    # count only: one pass, nothing but lims and info
    counts, cinfo = eng.search_range_counts(q, t, "l2")
    np.testing.assert_array_equal(counts, np.diff(lims))
    np.testing.assert_array_equal(cinfo, [total, info[1], total, 0])
    rc = lib.ef_search_range(eng._h, q.ctypes.data, b, N.EF_METRIC_L2, t, None, out_l.ctypes.data, out_r.ctypes.data,
                             out_s.ctypes.data, 0, info.ctypes.data, 0)
    assert rc == N.EF_OK and info[2] == total and (out_r[fit:] == -7).all()
    # the default capacity grows to the total when 16 hits per probe and 65 536 are not enough
    r = eng.search_range(q, t, "l2")
    assert r.complete and r.capacity == 65536 >= total
    _check(r, ref, q, g, "l2", t)


def test_default_capacity_grows_to_the_total(eng):
    n, b = 1100, 70  # 77 000 hits: past the starting capacity of 65 536
    v = np.random.default_rng(2).standard_normal(16).astype(np.float32)
    g, q = np.tile(v, (n, 1)), np.tile(v, (b, 1))
    r = _run(eng, g, q, "l2", 0.5)
    assert r.info[0] == n * b > 65536 and r.capacity == n * b and r.complete and r.info[2] == 0
    np.testing.assert_array_equal(r.rows.reshape(b, n), np.tile(np.arange(n), (b, 1)))


# ------------------------------------------------------------------ device tensors, determinism
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_device_tensors_on_a_callers_stream(eng, metric):
    import torch
    g, q, t, ref = blob_case(700, 130, metric)
    host = _run(eng, g, q, metric, t)
    _check(host, ref, q, g, metric, t)
    stream = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(stream):
        qd = torch.as_tensor(q.copy(), device="cuda")
        for _ in range(2):
            r = eng.search_range(qd, t, metric, max_results=int(ref[0][-1]))
            assert r.on_device and r.complete is None and r.lims.dtype == torch.int64
            assert r.rows.dtype == torch.int64 and r.scores.dtype == torch.float32
            outs.append(r)
        counts, cinfo = eng.search_range_counts(qd, t, metric)
        assert counts.is_cuda and cinfo.is_cuda
    stream.synchronize()
    for r in outs:
        h = r.host()
        assert h.complete
        for x, y in zip((h.lims, h.rows, h.scores, h.info), (host.lims, host.rows, host.scores, host.info)):
            assert x.tobytes() == y.tobytes()  # byte-equal to the host call, and run to run
    np.testing.assert_array_equal(counts.cpu().numpy(), np.diff(ref[0]))


# ------------------------------------------------------------------ state and arguments
def test_state_and_arguments(eng):
    import torch
    from eigenface import Engine
    lib = N.lib()
    q = np.random.default_rng(2).standard_normal((4, 5)).astype(np.float32)
    lims, rows, scores = np.zeros(5, np.int64), np.zeros(8, np.int64), np.zeros(8, np.float32)
    info = np.zeros(4, np.int64)

    def call(h, qp=q.ctypes.data, b=4, metric=N.EF_METRIC_L2, t=1.0, lp=lims.ctypes.data, rp=rows.ctypes.data,
             sp=scores.ctypes.data, cap=8, ip=info.ctypes.data):
        return lib.ef_search_range(h, qp, b, metric, t, None, lp, rp, sp, cap, ip, 0)
    with Engine(0) as fresh:
        with pytest.raises(RuntimeError):
            fresh.search_range(q, 1.0)
        assert call(fresh._h) == N.EF_E_STATE
        # an empty gallery: EF_OK, lims and info all zero
        fresh.set_gallery(np.zeros((0, 5), np.float32))
        lims[:], info[:] = -1, -1
        assert call(fresh._h) == N.EF_OK and (lims == 0).all() and (info == 0).all()
        r = fresh.search_range(q, 1.0)
        assert r.complete and r.rows.size == 0 and (r.counts == 0).all()
    g = np.random.default_rng(3).standard_normal((8, 5)).astype(np.float32)
    eng.set_gallery(g)
    assert call(eng._h, t=float("nan")) == N.EF_E_INVALID
    assert call(eng._h, metric=7) == N.EF_E_INVALID
    assert call(eng._h, lp=None) == N.EF_E_INVALID
    assert call(eng._h, ip=None) == N.EF_E_INVALID
    assert call(eng._h, cap=-1) == N.EF_E_INVALID
    assert call(eng._h, sp=None) == N.EF_E_INVALID  # rows without scores
    assert call(eng._h, qp=None) == N.EF_E_INVALID
    assert call(eng._h, b=-1) == N.EF_E_INVALID
    assert call(eng._h) == N.EF_OK
    lims[:] = -1
    assert call(eng._h, b=0) == N.EF_OK and lims[0] == 0 and (lims[1:] == -1).all()  # b = 0 writes lims[0] alone
    assert call(eng._h, rp=None, sp=None) == N.EF_OK  # count only
    with pytest.raises(ValueError):
        eng.search_range(q, float("nan"))
    with pytest.raises(ValueError):
        eng.search_range(q, 1.0, max_results=-1)
    with pytest.raises(ValueError):
        eng.search_range(q[:, :4], 1.0)
    with pytest.raises(ValueError):
        eng.search_range(q, 1.0, exclude_rows=np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        eng.search_range(q, 1.0, out=(rows, scores))  # out is for device input
    qd = torch.as_tensor(q, device="cuda")
    with pytest.raises(ValueError):
        eng.search_range(qd, 1.0, out=(torch.zeros(8, dtype=torch.int32, device="cuda"),
                                       torch.zeros(8, dtype=torch.float32, device="cuda")))
    with pytest.raises(ValueError):
        eng.search_range(qd, 1.0, out=(torch.zeros(8, dtype=torch.int64, device="cuda"),
                                       torch.zeros(9, dtype=torch.float32, device="cuda")))
    # the timer covers the call
    eng.timing(True)
    eng.timing_reset()
    eng.search_range(q, 1.0)
    ms, launches = eng.timing_get("range")
    eng.timing(False)
    assert launches == 1 and ms > 0.0


# ------------------------------------------------------------------ the layers above
def test_neighbors_layer(eng):
    """radius_neighbors on an engine, two row shards merged into the whole, and the vote."""
    g, q, t, ref = blob_case(300, 100, "cosine")
    whole = nb.radius_neighbors(g, q, t, "cosine", engine=eng)
    _check(whole, ref, q, g, "cosine", t)
    parts = []
    for lo, hi in ((0, 170), (170, 300)):
        eng.set_gallery(g[lo:hi], global_offset=lo)
        parts.append(eng.search_range(q, t, "cosine"))
    merged = nb.merge_range(parts)
    for x, y in zip((merged.lims, merged.rows, merged.scores), (whole.lims, whole.rows, whole.scores)):
        assert x.tobytes() == y.tobytes()
    assert merged.info[0] == whole.info[0]
    eng.set_gallery(g)
    _, cls = cu.blobs(300, 100, 5, 100 * 300 + 100)
    lab, votes, hits = nb.label_votes(whole, cls)
    np.testing.assert_array_equal(hits, np.diff(ref[0]))
    p = 0
    seg = ref[1][ref[0][p]:ref[0][p + 1]]
    assert votes[p] == np.bincount(cls[seg]).max() and lab[p] == np.bincount(cls[seg]).argmax()


def test_recognize_range_projects_first(eng):
    import torch
    rng = np.random.default_rng(9)
    d, k, n = 96, 24, 300
    mean = rng.uniform(0, 255, d)
    w = np.linalg.qr(rng.standard_normal((d, k)))[0]
    eng.set_model(mean, w)
    faces = rng.integers(0, 256, (n, d)).astype(np.uint8)
    feats = eng.project(faces)
    eng.set_gallery(feats)
    probes = faces[[5, 17, 250]]
    r = eng.recognize_range(probes, 1e-3, "l2")
    same = eng.search_range(eng.project(probes), 1e-3, "l2")
    assert r.rows.tobytes() == same.rows.tobytes() and r.lims.tobytes() == same.lims.tobytes()
    assert [list(r.of(i)[0]) for i in range(3)] == [[5], [17], [250]]
    rd = eng.recognize_range(torch.as_tensor(probes, device="cuda"), 1e-3, "l2", max_results=16)
    assert rd.on_device and rd.host().rows.tobytes() == r.rows.tobytes()


# ------------------------------------------------------------------ work items of several tiles
def _differs_from_tile_to_tile(x):
    """An input condition: a per-row value taken from the tile before or after is another value."""
    assert (x[:-128] != x[128:]).mean() > 0.9


@functools.lru_cache(maxsize=None)
def lattice_case(k):
    """4229 lattice rows (34 tiles, 5 rows in the last) and 8192 probes, each a copy of a random
    row: a quarter unchanged, a quarter with coordinate 6 flipped, a quarter with coordinate 7
    flipped, a quarter moved by +2 in coordinate 0 (no lattice point: nothing within t = 1)."""
    n, b = 4229, 8192
    g = cu.lattice(n, k, 7 * k)
    rng = np.random.default_rng(1000 + k)
    q = g[rng.integers(0, n, b)].copy()
    kind = np.arange(b) % 4
    rng.shuffle(kind)
    q[kind == 1, 6] = 1 - q[kind == 1, 6]
    q[kind == 2, 7] = 1 - q[kind == 2, 7]
    q[kind == 3, 0] += 2
    ref = ru.reference(q, g, "l2", 1.0, gram=True)  # integers: the Gram form is exact
    lims, rows, scores = ref
    counts = np.diff(lims)
    assert lims[-1] == {16: 20381, 40: 19938}[k] and counts.max() <= 11 and (counts == 0).sum() == 2048
    assert set(np.unique(scores)) == {0.0, 1.0} and (scores == 1.0).sum() == {16: 13694, 40: 13312}[k]
    # every tile, both lane halves and all four row blocks are hit
    assert np.unique(rows // 128).size == 34 and (rows >= 33 * 128).sum() >= 10
    assert set(np.unique((rows % 8) // 4)) == {0, 1} and set(np.unique((rows % 128) // 32)) == {0, 1, 2, 3}
    multi = np.flatnonzero(counts > 1)
    spans = [np.unique(rows[lims[p]:lims[p + 1]] // 256).size > 1 for p in multi]
    assert np.mean(spans) > 0.95  # hits in more than one two-tile chunk: the running offset matters
    # scores 0 and 2 are decided by the fp32 scan, score 1 = t lies inside the band
    assert ru.delta(q, g, "l2", 1.0).max() < 0.5
    _differs_from_tile_to_tile((g.astype(np.float64) ** 2).sum(axis=1))
    _freeze(g, q, *ref)
    return g, q, ref


@pytest.mark.parametrize("k", (16, 40))
def test_work_items_of_several_tiles(eng, k):
    """The planner's branch of two row tiles per item, the last item ending on the 5-row tile; the
    aux values of the second tile sit in the odd slot, and a probe's running offset carries from
    tile to tile.  k = 16 is one slice per tile, k = 40 (kp = 64) four."""
    n, b = 4229, 8192
    chunks, tpi = nb.search_range_plan(b, n, cu.kp_of(k))
    assert tpi >= 2 and (chunks, tpi) == (17, 2) and n - 33 * 128 == 5 and (chunks - 1) * tpi + 2 == 34
    assert cu.kp_of(k) // 16 == (1 if k == 16 else 4)
    g, q, ref = lattice_case(k)
    r = _run(eng, g, q, "l2", 1.0)
    _check(r, ref, q, g, "l2", 1.0)
    assert r.info[1] >= (ref[2] == 1.0).sum()  # the pairs at t itself are settled in fp64
    np.testing.assert_array_equal(r.scores, ref[2].astype(np.float32))


# ------------------------------------------------------------------ offset scan past one block
def test_offset_scan_carries_past_256_blocks(eng):
    """b = 65836: 258 blocks of 256 probes, so range_scan_kernel runs a second round on the
    running total of the first; there are hits on both sides of the carry."""
    n, b, k = 200, 65836, 16
    line = 65536
    assert (b + 255) // 256 == 258
    g = cu.lattice(n, k, 5)
    rng = np.random.default_rng(6)
    q = g[rng.integers(0, n, b)].copy()
    q[rng.random(b) < 0.3, 0] += 2  # probes without a hit, on both sides too
    ref = ru.reference(q, g, "l2", 1.0, gram=True)
    lims = ref[0]
    counts = np.diff(lims)
    assert 0 < lims[line] < lims[-1] and (counts[line:] > 0).any() and (counts[line:] == 0).any()
    assert (counts[:line] == 0).any() and np.unique(counts[line:]).size > 2
    r = _run(eng, g, q, "l2", 1.0)
    _check(r, ref)
    np.testing.assert_array_equal(r.scores, ref[2].astype(np.float32))
