"""Range search, the parts that need no GPU: RangeResult, merge_range, label_votes and by_score on
hand-made data, the host-only planner, the symbols, and the numpy reference against a plain loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import cluster_util as cu
import range_util as ru
from eigenface import _native as N
from eigenface import neighbors as nb

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _result(segments, metric="l2", capacity=None, info1=0):
    """A RangeResult from per-probe lists of (row, score)."""
    lims = np.zeros(len(segments) + 1, np.int64)
    np.cumsum([len(s) for s in segments], out=lims[1:])
    rows = np.array([r for s in segments for r, _ in s], np.int64)
    scores = np.array([v for s in segments for _, v in s], np.float32)
    total = int(lims[-1])
    cap = total if capacity is None else capacity
    return nb.RangeResult(lims, rows, scores, np.array([total, info1, 0, 0], np.int64), metric, cap)


# ------------------------------------------------------------------ the result object
def test_range_result_accessors():
    r = _result([[(2, 0.5), (7, 0.25)], [], [(0, 1.0), (3, 0.0), (9, 0.75)]])
    assert r.n_probes == 3 and r.complete is True and not r.on_device
    np.testing.assert_array_equal(r.counts, [2, 0, 3])
    rows, scores = r.of(2)
    np.testing.assert_array_equal(rows, [0, 3, 9])
    np.testing.assert_array_equal(scores, np.array([1.0, 0.0, 0.75], np.float32))
    assert r.of(1)[0].size == 0
    probe, rows, scores = r.pairs()
    np.testing.assert_array_equal(probe, [0, 0, 2, 2, 2])
    np.testing.assert_array_equal(rows, [2, 7, 0, 3, 9])
    assert r.host() is not r and r.host().complete


def test_by_score_orders_best_first_with_ties_by_row():
    r = _result([[(2, 0.5), (7, 0.25), (8, 0.5)], [(1, 3.0)]])
    s = r.by_score()
    np.testing.assert_array_equal(s.lims, r.lims)
    np.testing.assert_array_equal(s.rows, [7, 2, 8, 1])  # l2: the lowest distance first; 2 before 8
    np.testing.assert_array_equal(r.rows, [2, 7, 8, 1])  # the original is untouched
    c = _result([[(2, 0.5), (7, 0.25), (8, 0.5), (9, 0.9)]], metric="cosine").by_score()
    np.testing.assert_array_equal(c.rows, [9, 2, 8, 7])  # cosine: the highest similarity first
    np.testing.assert_array_equal(c.scores, np.array([0.9, 0.5, 0.5, 0.25], np.float32))


def test_incomplete_result():
    """Capacity 4: the segments ending at 2 and 2 fit, the one ending at 5 was not written."""
    r = _result([[(2, 0.5), (7, 0.25)], [], [(0, 1.0), (3, 0.0), (9, 0.75)]], capacity=4)
    r.rows, r.scores = r.rows[:2], r.scores[:2]
    assert r.complete is False
    np.testing.assert_array_equal(r.of(0)[0], [2, 7])
    with pytest.raises(ValueError):
        r.of(2)
    probe, rows, _ = r.pairs()
    np.testing.assert_array_equal(probe, [0, 0])
    np.testing.assert_array_equal(rows, [2, 7])
    with pytest.raises(ValueError):
        nb.merge_range([r])
    with pytest.raises(ValueError):
        nb.label_votes(r, np.zeros(10, np.int64))


def test_merge_range_concatenates_per_probe():
    a = _result([[(0, 0.5), (3, 0.1)], [], [(2, 0.2)]], info1=1)
    b = _result([[(10, 0.3)], [(11, 0.4), (12, 0.6)], []], info1=2)
    c = _result([[], [(25, 0.9)], [(20, 0.7), (29, 0.8)]])
    m = nb.merge_range([a, b, c])
    np.testing.assert_array_equal(m.lims, [0, 3, 6, 9])
    np.testing.assert_array_equal(m.rows, [0, 3, 10, 11, 12, 25, 2, 20, 29])
    np.testing.assert_array_equal(m.scores, np.array([0.5, 0.1, 0.3, 0.4, 0.6, 0.9, 0.2, 0.7, 0.8], np.float32))
    np.testing.assert_array_equal(m.info, [9, 3, 0, 0])
    assert m.complete and m.metric == "l2"
    for p in range(3):
        assert (np.diff(m.of(p)[0]) > 0).all()  # still ascending
    with pytest.raises(ValueError):
        nb.merge_range([b, a])  # not in ascending offset order
    with pytest.raises(ValueError):
        nb.merge_range([a, _result([[(10, 0.3)]])])  # another probe count
    with pytest.raises(ValueError):
        nb.merge_range([a, _result([[], [], []], metric="cosine")])
    with pytest.raises(ValueError):
        nb.merge_range([])


def test_label_votes():
    labels = np.array([5, 5, 7, 7, 7, 9, 9, 3], np.int64)  # by global row
    r = _result([
        [(0, 0.4), (1, 0.5), (2, 0.1)],            # 5 twice, 7 once
        [],                                        # no hit
        [(0, 0.4), (2, 0.3), (5, 0.2), (6, 0.9)],  # 5 once, 7 once, 9 twice
        [(1, 0.6), (3, 0.2), (7, 0.2)],            # three labels tie: best score 0.2 at rows 3 and 7, row 3 first
        [(0, 0.3), (1, 0.1), (2, 0.2), (4, 0.5)],  # 5 and 7 tie at two: the best hit is row 1 (label 5)
    ])
    lab, votes, hits = nb.label_votes(r, labels)
    np.testing.assert_array_equal(lab, [5, -1, 9, 7, 5])
    np.testing.assert_array_equal(votes, [2, 0, 2, 1, 2])
    np.testing.assert_array_equal(hits, [3, 0, 4, 3, 4])
    # cosine: the best hit is the highest similarity
    c = _result([[(0, 0.3), (2, 0.8)]], metric="cosine")
    assert nb.label_votes(c, labels)[0][0] == 7


# ------------------------------------------------------------------ the planner
def _plan_restated(b, n):
    """range_plan restated: about 2048 (chunk, probe tile) items."""
    ptiles = (b + 255) // 256 * 2
    tiles = (n + 127) // 128
    if not ptiles or not tiles:
        return 0, 0
    parts = min(max(1, -(-2048 // ptiles)), tiles)
    tpi = -(-tiles // parts)
    return -(-tiles // tpi), tpi


@pytest.mark.parametrize("b", (1, 77, 256, 257, 4096, 8192, 70000, 600000))
@pytest.mark.parametrize("n", (1, 127, 128, 129, 4229, 100003, 1000000))
def test_plan_covers_every_tile_once(b, n):
    chunks, tpi = nb.search_range_plan(b, n, 128)
    assert (chunks, tpi) == _plan_restated(b, n)
    tiles = (n + 127) // 128
    seen = np.zeros(tiles, np.int32)
    for c in range(chunks):
        t0, t1 = c * tpi, min((c + 1) * tpi, tiles)
        assert t0 < t1  # no empty chunk: every (chunk, probe tile) item publishes its counts
        seen[t0:t1] += 1
    assert (seen == 1).all()


def test_plan_at_the_shapes_of_the_gpu_tests():
    # work items of several tiles: 34 row tiles with 5 rows in the last, two tiles per item
    assert nb.search_range_plan(8192, 4229, 16) == (17, 2) and 4229 - 33 * 128 == 5
    assert nb.search_range_plan(8192, 4229, 64) == (17, 2)
    # the small cases are one tile per item
    for n, b in ((129, 77), (700, 77), (257, 129), (300, 70)):
        chunks, tpi = nb.search_range_plan(b, n, 16)
        assert tpi == 1 and chunks == (n + 127) // 128
    # the offset scan's second level carries past 256 blocks of 256 probes
    assert (65836 + 255) // 256 == 258 and nb.search_range_plan(65836, 200, 16) == (2, 1)


def test_plan_rejects_bad_sizes():
    lib = N.lib()
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    ra, rb = ctypes.byref(a), ctypes.byref(b)
    assert lib.ef_search_range_plan(-1, 10, 128, ra, rb) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(10, -1, 128, ra, rb) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(10, 2 ** 31, 128, ra, rb) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(10, 10, 0, ra, rb) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(10, 10, 24, ra, rb) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(10, 10, 128, None, rb) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(10, 10, 128, ra, None) == N.EF_E_INVALID
    assert lib.ef_search_range_plan(0, 10, 128, ra, rb) == N.EF_OK and (a.value, b.value) == (0, 0)
    assert lib.ef_search_range_plan(10, 0, 128, ra, rb) == N.EF_OK and (a.value, b.value) == (0, 0)
    with pytest.raises(N.EigenfaceError):
        nb.search_range_plan(10, 10, 24)


# ------------------------------------------------------------------ symbols and prototypes
def test_symbols_and_prototypes():
    lib = N.lib()
    for name in ("ef_search_range", "ef_search_range_plan"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    assert N._SIGS["ef_search_range"] == ([vp, vp, i64, i32, ctypes.c_double, vp, vp, vp, vp, i64, vp, u32],
                                          ctypes.c_int)
    assert N._SIGS["ef_search_range_plan"] == ([i64, i64, i32, ctypes.POINTER(i64), ctypes.POINTER(i64)], ctypes.c_int)
    with open(os.path.join(ROOT, "include", "eigenface.h")) as f:
        hdr = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    assert ("int ef_search_range(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric, double threshold, "
            "const int64_t* exclude_rows , int64_t* lims , int64_t* rows , float* scores , int64_t cap, "
            "int64_t* info , uint32_t flags);") in flat
    assert ("int ef_search_range_plan(int64_t b, int64_t n, int32_t kp, int64_t* n_chunks, "
            "int64_t* tiles_per_item);") in flat
    assert "#define EF_API_VERSION 7" in hdr
    assert re.search(r"#define EF_KERNEL_RANGE 13\b", hdr) and N.EF_KERNEL_RANGE == 13
    import eigenface
    for name in ("RangeResult", "radius_neighbors", "merge_range", "label_votes", "search_range_plan"):
        assert hasattr(eigenface, name) and name in eigenface.__all__
    for name in ("search_range", "search_range_counts", "recognize_range"):
        assert hasattr(eigenface.Engine, name)


# ------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_reference_against_a_plain_loop(metric):
    g, _ = cu.blobs(203, 9, 4, 31)
    g = g.copy()
    rng = np.random.default_rng(8)
    q = (g[rng.integers(0, 203, 37)] + 0.3 * rng.standard_normal((37, 9))).astype(np.float32)
    g[17] = 0.0
    g[40, 2] = np.nan
    q[5] = 0.0
    q[9, 0] = np.inf
    excl = np.full(37, -1, np.int64)
    excl[:12] = rng.integers(1000, 1203, 12)
    excl[3] = 999
    excl[4] = 1203
    v = ru.finite_scores(q, g, metric)
    t, _ = ru.widest_gap(v, 3.0 * 9, 5.0 * 9) if metric == "l2" else ru.widest_gap(v, 0.3, 0.9)
    got = ru.reference(q, g, metric, t, excl, offset=1000)
    want = ru.brute_force(q, g, metric, t, excl, offset=1000)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-13, atol=1e-13)
    assert 0 < got[0][-1] < 37 * 203 and got[0][10] == got[0][9]  # the non-finite probe has no hit
    assert 1040 not in got[1]
    for p in range(37):
        seg = got[1][got[0][p]:got[0][p + 1]]
        assert (np.diff(seg) > 0).all() and excl[p] not in seg
    # the Gram form agrees where it is exact: integers
    gi, qi = np.rint(g[:50].copy()), np.rint(q[:8].copy())
    gi[~np.isfinite(gi)] = 0
    qi[~np.isfinite(qi)] = 0
    if metric == "l2":
        a = ru.reference(qi, gi, "l2", 40.0, gram=True)
        c = ru.reference(qi, gi, "l2", 40.0)
        for x, y in zip(a, c):
            np.testing.assert_array_equal(x, y)


def test_reference_delta_is_the_headers_formula():
    g = np.array([[3.0, 4.0], [0.0, 1.0]], np.float32)  # max |g| = 5
    q = np.array([[6.0, 8.0], [0.0, 0.0]], np.float32)  # |q| = 10, 0
    t = 0.1  # not an fp32 number
    terr = abs(float(np.float32(t)) - t)
    u = 2.0 ** -24
    d = ru.delta(q, g, "l2", t)
    assert d[0] == 2 * ((16 + 4) * u * 1.01 * (2 * 10 * 5 + 25) + 4 * u * 15 ** 2) + terr
    assert d[1] == 2 * ((16 + 4) * u * 1.01 * 25 + 4 * u * 25) + terr
    assert (ru.delta(q, g, "cosine", t) == 2 * (16 + 12) * u * 1.01 + terr).all()
