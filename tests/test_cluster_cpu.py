"""Gallery clustering, the parts that need no GPU: the host-only planner's tile coverage, the
symbols and prototypes, the pair-count metrics and the numpy reference itself."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import cluster_util as cu
from eigenface import _native as N
from eigenface import cluster as ec

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------------ the planner
@pytest.mark.parametrize("kp", (16, 128, 256, 640))
@pytest.mark.parametrize("n", (1, 127, 128, 129, 257, 1000, 100003))
def test_schedule_covers_every_tile_pair_once(n, kp):
    items = ec.cluster_schedule(n, kp)
    tiles = (n + 127) // 128
    assert items.shape[1] == 3 and items.shape[0] >= 1
    t0, t1, pt = items.T
    assert (t0 >= 0).all() and (t0 < t1).all() and (t1 <= pt + 1).all() and (pt < tiles).all()
    seen = np.zeros((tiles, tiles), np.int32)  # [probe tile][row tile]
    for a, b, p in items:
        seen[p, a:b] += 1
    want = np.tril(np.ones((tiles, tiles), np.int32))  # row tile <= probe tile
    np.testing.assert_array_equal(seen, want)


def test_schedule_rejects_bad_sizes():
    cnt = ctypes.c_int32(0)
    lib = N.lib()
    assert lib.ef_cluster_schedule(-1, 128, None, 0, ctypes.byref(cnt)) == N.EF_E_INVALID
    assert lib.ef_cluster_schedule(10, 0, None, 0, ctypes.byref(cnt)) == N.EF_E_INVALID
    assert lib.ef_cluster_schedule(10, 24, None, 0, ctypes.byref(cnt)) == N.EF_E_INVALID
    assert lib.ef_cluster_schedule(10, 128, None, 0, None) == N.EF_E_INVALID
    assert lib.ef_cluster_schedule(0, 128, None, 0, ctypes.byref(cnt)) == N.EF_OK and cnt.value == 0
    # a short buffer is filled as far as it goes and the total is still reported
    few = np.full((2, 3), -1, np.int64)
    assert lib.ef_cluster_schedule(1000, 128, few.ctypes.data, 2, ctypes.byref(cnt)) == N.EF_OK
    assert cnt.value == ec.cluster_schedule(1000, 128).shape[0] > 2
    np.testing.assert_array_equal(few, ec.cluster_schedule(1000, 128)[:2])


# ------------------------------------------------------------------ symbols and prototypes
def test_symbols_and_prototypes():
    lib = N.lib()
    for name in ("ef_gallery_cluster", "ef_cluster_schedule"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    assert N._SIGS["ef_gallery_cluster"] == ([vp, i32, ctypes.c_double, i32, vp, vp, vp, u32], ctypes.c_int)
    assert N._SIGS["ef_cluster_schedule"] == ([i64, i32, vp, i32, ctypes.POINTER(i32)], ctypes.c_int)
    with open(os.path.join(ROOT, "include", "eigenface.h")) as f:
        hdr = f.read()
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int ef_gallery_cluster(ef_ctx* ctx, int32_t metric, double threshold, int32_t min_samples, "
            "int32_t* labels , int32_t* degree , int64_t* info , uint32_t flags);") in flat
    assert ("int ef_cluster_schedule(int64_t n, int32_t kp, int64_t* items_out , int32_t max_items, "
            "int32_t* n_items);") in flat
    assert "#define EF_API_VERSION 7" in hdr
    assert re.search(r"#define EF_KERNEL_CLUSTER 12\b", hdr) and N.EF_KERNEL_CLUSTER == 12
    assert N.EF_CLUSTER_UNCONVERGED == 1 << 62 and "#define EF_CLUSTER_UNCONVERGED ((int64_t)1 << 62)" in hdr
    import eigenface
    for name in ("cluster_gallery", "cluster_faces", "pair_confusion", "pairwise_scores", "ClusterResult"):
        assert hasattr(eigenface, name) and name in eigenface.__all__
    assert hasattr(eigenface.Engine, "cluster_gallery")


# ------------------------------------------------------------------ pair counts
def _brute_confusion(true, pred):
    pred = list(pred)
    fresh = max([p for p in pred if p >= 0], default=-1) + 1
    for i, p in enumerate(pred):
        if p < 0:
            pred[i] = fresh
            fresh += 1
    tp = fp = fn = tn = 0
    for i, j in itertools.combinations(range(len(true)), 2):
        st, sp = true[i] == true[j], pred[i] == pred[j]
        tp += st and sp
        fp += sp and not st
        fn += st and not sp
        tn += not st and not sp
    return tp, fp, fn, tn


@pytest.mark.parametrize("seed", range(4))
def test_pair_confusion_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = 60
    true = rng.integers(0, 5, n)
    pred = rng.integers(-1, 7, n)
    assert (pred < 0).any()
    assert ec.pair_confusion(true, pred) == _brute_confusion(true, pred)
    assert sum(ec.pair_confusion(true, pred)) == n * (n - 1) // 2


def test_pair_confusion_edge_cases():
    assert ec.pair_confusion([], []) == (0, 0, 0, 0)
    assert ec.pair_confusion([3], [0]) == (0, 0, 0, 0)
    assert ec.pair_confusion(["a", "a", "b"], [0, 0, 1]) == (1, 0, 0, 2)
    assert ec.pair_confusion([0, 0, 0], [-1, -1, -1]) == (0, 0, 3, 0)  # noise rows are singletons
    assert ec.pairwise_scores([0, 0, 1, 1], [0, 0, 1, 1]) == {"precision": 1.0, "recall": 1.0, "f1": 1.0}
    s = ec.pairwise_scores([0, 0, 1, 1], [0, 0, 0, 0])
    assert s["precision"] == 2 / 6 and s["recall"] == 1.0
    with pytest.raises(ValueError):
        ec.pair_confusion([0, 1], [0])


def test_clustering_agreement_in_evaluate():
    from eigenface.evaluate import clustering_agreement
    r = clustering_agreement([0, 0, 1, 1, 2], [0, 0, 0, -1, -1])
    assert (r["tp"], r["fp"], r["fn"], r["tn"]) == _brute_confusion([0, 0, 1, 1, 2], [0, 0, 0, -1, -1])
    assert r["precision"] == 1 / 3 and r["recall"] == 1 / 2


def test_pair_confusion_against_sklearn():
    skm = pytest.importorskip("sklearn.metrics.cluster")
    rng = np.random.default_rng(7)
    true = rng.integers(0, 6, 300)
    pred = rng.integers(0, 9, 300)
    m = skm.pair_confusion_matrix(true, pred)  # ordered pairs: twice ours
    tp, fp, fn, tn = ec.pair_confusion(true, pred)
    assert (2 * tn, 2 * fp, 2 * fn, 2 * tp) == (m[0, 0], m[0, 1], m[1, 0], m[1, 1])


# ------------------------------------------------------------------ the reference itself
def _random_graph(seed, n=150, p=0.012):
    rng = np.random.default_rng(seed)
    a = np.triu(rng.random((n, n)) < p, 1)
    return a | a.T


@pytest.mark.parametrize("seed", range(3))
def test_reference_components_brute_force(seed):
    adj = _random_graph(seed)
    n = adj.shape[0]
    reach = adj | np.eye(n, dtype=bool)
    for _ in range(8):  # closure by squaring: paths up to 256
        reach = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
    want = np.array([np.flatnonzero(reach[i])[0] for i in range(n)])
    got = cu.components(adj)
    np.testing.assert_array_equal(got, want)
    assert 1 < np.unique(got).size < n


def test_reference_components_against_scipy():
    csg = pytest.importorskip("scipy.sparse.csgraph")
    sp = pytest.importorskip("scipy.sparse")
    for seed in range(3):
        adj = _random_graph(seed, 400, 0.004)
        nc, lab = csg.connected_components(sp.csr_matrix(adj), directed=False)
        root = cu.components(adj)
        assert np.unique(root).size == nc
        # the same partition: a bijection between scipy's labels and our roots
        assert len(set(zip(lab.tolist(), root.tolist()))) == nc
        assert (root <= np.arange(400)).all()


def test_canonical_relabelling():
    root = np.array([0, 0, 2, 0, 2, 5, -1, 5])
    np.testing.assert_array_equal(cu.canonical(root), [0, 0, 1, 0, 1, 2, -1, 2])
    # numbered by the lowest member row, whatever the order the clusters were found in
    perm = np.array([5, 5, 1, 1, 0, 0])
    np.testing.assert_array_equal(cu.canonical(np.array([4, 4, 2, 2, 0, 0])[np.argsort(perm, kind="stable")]),
                                  [0, 0, 1, 1, 2, 2])


def test_reference_density_rule():
    # points on a line, linked within 0.96: rows 0-2 and 6-8 are tight groups, rows 3 and 5 lie
    # between them (3 reaches row 2, 5 reaches rows 2 and 6), row 4 is isolated
    x = np.array([0.0, 0.1, 0.2, 1.1, 9.0, 1.15, 2.1, 2.2, 2.3, 3.2])  # row 9 reaches row 8 only
    g = np.zeros((10, 4), np.float32)
    g[:, 0] = x
    lab, deg, info = cu.reference(g, "l2", 0.96 ** 2, 1)
    assert info[0] == 2 and info[1] == 0 and lab[4] == 1 and (np.delete(lab, 4) == 0).all()
    lab, deg, info = cu.reference(g, "l2", 0.96 ** 2, 3)
    # the rule, from the degrees themselves: noise, and the lowest-index linked core row
    core = deg + 1 >= 3
    assert (~core & (lab >= 0)).any()
    assert not core[4] and lab[4] == -1 and info[1] == (lab < 0).sum()
    for r in np.flatnonzero(~core & (lab >= 0)):
        d2 = (x - x[r]) ** 2
        nb = np.flatnonzero((d2 <= 0.96 ** 2) & core & (np.arange(10) != r))
        assert lab[r] == lab[nb[0]]


# ------------------------------------------------------------------ the lattice and its hash reference
@pytest.mark.parametrize("min_samples", (1, 3, 5))
@pytest.mark.parametrize("n,k", ((700, 16), (701, 40)))
def test_lattice_reference_equals_the_dense_reference(n, k, min_samples):
    g = cu.lattice(n, k, n + k)
    s = cu.pair_scores(g, "l2")
    v = cu.upper(s)
    assert (s == np.rint(s)).all() and set(np.unique(v[v < 16])) == {0.0, 1.0, 2.0}
    dense = cu.reference(g, "l2", 1.0, min_samples, s)
    lab, deg, info = dense
    core = deg + 1 >= min_samples
    assert (np.bincount(lab[lab >= 0]) > 1).any()  # clusters of several rows
    if min_samples > 1:
        assert (~core & (lab >= 0)).any() and (lab < 0).any() and info[1] > 0  # attached rows, noise rows
    assert cu.lattice_unit_pairs(g) == int((v == 1.0).sum())
    for got, want in zip(cu.lattice_reference(g, min_samples), dense):
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got, want)
    # the duplicates alone: the graph of score 0
    for got, want in zip(cu.lattice_reference(g, min_samples, unit_steps=False),
                         cu.reference(g, "l2", 0.0, min_samples, s)):
        np.testing.assert_array_equal(got, want)


def test_max_cosine_between_points_equals_the_dense_maximum():
    g = cu.lattice(700, 16, 716)
    s = cu.pair_scores(g, "cosine")
    apart = cu.pair_scores(g, "l2") > 0
    assert cu.max_cosine_between_points(g, block=64) == pytest.approx(s[apart].max(), abs=1e-15)
    assert (s[~apart] >= 1 - 1e-15).all()


# the large galleries of test_gpu_cluster.py: (n, k)
LATTICE_SIZES = ((11530, 16), (11530, 40), (65836, 16))


@pytest.mark.parametrize("n,k", LATTICE_SIZES)
def test_large_lattices_reach_items_of_several_tiles(n, k):
    """What test_gpu_cluster.py relies on at these sizes, from the planner alone."""
    tiles = (n + 127) // 128
    assert n % 128 != 0
    # the link pass: an item of two or more row tiles that holds its own diagonal tile, not first
    t0, t1, pt = ec.cluster_schedule(n, cu.kp_of(k)).T
    assert int((t1 - t0).max()) == max(1, tiles * (tiles + 1) // 2 // 2048) >= 2
    late_diagonal = (t1 - t0 >= 2) & (pt > t0) & (pt < t1)
    assert late_diagonal.any() and (t0[late_diagonal] > 0).any()
    # the count pass sweeps the full square (cluster_tiles_per_item(tiles, true) restated): the
    # ragged last tile is a later tile of its item
    tpc = min(tiles, max(1, tiles * tiles // 2048))
    assert tpc >= 2 and (tiles - 1) % tpc != 0
    # the label scan carries a running total between rounds of 256 blocks of 256 rows
    assert ((n + 255) // 256 > 256) == (n == 65836)
