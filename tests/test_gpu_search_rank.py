"""Identification rank on the GPU (ef_search_rank) against the numpy fp64 reference
of tests/rank_util.py.  Every generator asserts its own conditions on the reference before the GPU
is asked: by default that no other identity's best score lies within 1e-9 of the largest score
of the probe's tau (a last-ulp difference between numpy's formula and the kernel's fp64 score
then changes no decision); the cases built on exact ties use bit-identical rows or small-integer
features, whose scores are exact in both."""
import functools

import numpy as np
import pytest

import cluster_util as cu
import rank_util as rk
from eigenface import _native as N
from eigenface import evaluate as ev

pytestmark = pytest.mark.gpu

DEFAULT_BUDGET = 256 << 20


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _load(eng, g, lab, offset=0):
    eng.set_gallery(g, global_offset=offset)
    eng.set_gallery_labels(lab)


def _rank(eng, q, pl, metric, exclude=None, **kw):
    better, gen, info = eng.search_rank(q, pl, exclude, metric, **kw)
    assert better.dtype == np.int32 and better.shape == (q.shape[0],)
    assert gen.dtype == np.dtype(N.MATCH_DTYPE) and gen.shape == (q.shape[0],)
    assert info.dtype == np.int64 and info.shape == (4,) and info[3] == 0
    return better, gen, info


def _check(eng, g, lab, q, pl, metric, ref, exclude=None, offset=0):
    """better exactly the reference's; the genuine records those of the labelled SAME search, and
    their rows the reference's; info[0] inside the bounds delta_p gives; info[2] = C."""
    _load(eng, g, lab, offset)
    better, gen, info = _rank(eng, q, pl, metric, exclude)
    np.testing.assert_array_equal(better, ref["better"])
    want = eng.search_labelled_matches(q, pl, "same", exclude, metric)
    assert gen.tobytes() == want.tobytes()
    has = gen["key"] != N.EF_KEY_NONE
    np.testing.assert_array_equal(np.where(has, gen["key"] & 0xFFFFFFFF, -1), ref["row_gen"])
    assert info[2] == np.unique(lab).size and info[1] == 1
    lo, hi = rk.settled_bounds(ref, rk.delta(q, g, metric, ref["tau"]))
    assert lo <= info[0] <= hi, (lo, int(info[0]), hi)
    return better, gen, info


# ------------------------------------------------------------------ 1. blob galleries
BLOBS = ((129, 8), (300, 100), (700, 130), (513, 640))


@functools.lru_cache(maxsize=None)
def blob_case(n, k, C, metric):
    g, lab, centres, names = rk.blobs(n, k, C, 1000 * n + 10 * k + C)
    rng = np.random.default_rng(n + k + C)
    ident = rng.integers(0, C, 77)
    q = (centres[ident] + rng.standard_normal((77, k))).astype(np.float32)
    pl = names[ident]
    ref = rk.reference(q, g, lab, pl, metric)
    rel = rk.clear_margins(ref)
    vals = np.unique(ref["better"])
    assert vals.size >= 8 and vals[0] == 0 and (ref["better"] >= 0).all(), vals
    _freeze(g, lab, q, pl)
    return g, lab, q, pl, ref, rel


@pytest.mark.parametrize("metric", ("l2", "cosine"))
@pytest.mark.parametrize("C", (33, 65))
@pytest.mark.parametrize("n,k", BLOBS)
def test_blobs(eng, n, k, C, metric):
    g, lab, q, pl, ref, _ = blob_case(n, k, C, metric)
    _, _, info = _check(eng, g, lab, q, pl, metric, ref)
    assert info[0] > 0  # the genuine pair of every probe lies in its band: the fp64 settlement ran


# ------------------------------------------------------------------ 2. tile and word edges
ODD_LABELS = np.array([-7, 2 ** 31 - 1, 0, 1000003, -2 ** 31, 5, -1, 65536], np.int64)


def edge_labels(C):
    """C distinct int32 labels: negative, large, non-dense, in no order."""
    rng = np.random.default_rng(C)
    rest = rng.choice(np.arange(10 ** 6, 10 ** 6 + 10 ** 5), max(C - ODD_LABELS.size, 0), replace=False) * 977 % (2 ** 31)
    names = np.concatenate([ODD_LABELS, rest])[:C]
    assert np.unique(names).size == C
    return names.astype(np.int32)


@pytest.mark.parametrize("b", (1, 33, 129))
@pytest.mark.parametrize("n", (1, 2, 127, 128, 129, 257))
def test_tile_and_word_edges(eng, n, b):
    rng = np.random.default_rng(1000 * n + b)
    g = rng.standard_normal((n, 24)).astype(np.float32)
    pick = rng.integers(0, n, b)
    q = (g[pick] + 0.7 * rng.standard_normal((b, 24))).astype(np.float32)
    ran = 0
    for C in (1, 2, 31, 32, 33, 65):
        if C > n:
            continue
        names = edge_labels(C)
        lab = names[(np.arange(n) * 7 + 3) % C]
        assert np.unique(lab).size == C
        pl = lab[pick].copy()
        if b > 1:
            pl[-1] = 424242  # a label no row carries
            assert 424242 not in names
        for metric in ("l2", "cosine"):
            ref = rk.reference(q, g, lab, pl, metric)
            rk.clear_margins(ref)
            better, _, _ = _check(eng, g, lab, q, pl, metric, ref)
            if b > 1:
                assert better[-1] == -1
            if C == 1:
                assert (better[:-1] == 0).all() if b > 1 else (better == 0).all()
            ran += 1
    assert ran >= 2


# ------------------------------------------------------------------ 3. ties
@functools.lru_cache(maxsize=None)
def duplicate_case():
    """Small-integer rows (every score exact in fp64, here and on the GPU), 12 identities, and 24
    rows overwritten with a copy of a row of ANOTHER identity; the probes are those originals and
    copies themselves, under either label: the copy ties with the genuine row at distance 0 /
    cosine 1 and beats it only from a lower row index."""
    rng = np.random.default_rng(77)
    n, k, C = 260, 20, 12
    g = rng.integers(-6, 7, (n, k)).astype(np.float32)
    lab = (rng.permutation(n) % C).astype(np.int32) * 1000 - 3000
    src = rng.choice(n, 24, replace=False)
    dst = np.empty_like(src)
    taken = set(src.tolist())
    for i, a in enumerate(src):
        cand = [r for r in rng.permutation(n) if r not in taken and lab[r] != lab[a]]
        dst[i] = cand[0]
        taken.add(int(dst[i]))
        g[dst[i]] = g[a]
    q = np.concatenate([g[src], g[dst]])
    pl = np.concatenate([lab[src], lab[dst]])
    _freeze(g, lab, q, pl)
    return g, lab, q, pl, src, dst


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_duplicates_follow_the_row_index_rule(eng, metric):
    g, lab, q, pl, src, dst = duplicate_case()
    ref = rk.reference(q, g, lab, pl, metric, gram=True)
    # the genuine row of probe i is the row it copies, its twin of the other label ties exactly
    np.testing.assert_array_equal(ref["row_gen"], np.concatenate([src, dst]))
    twin = np.concatenate([dst, src])
    assert (ref["scores"][np.arange(48), twin] == ref["tau"]).all()
    lower = twin < ref["row_gen"]
    assert 8 <= lower.sum() <= 40  # both sides of row_gen
    m = ref["margin"]
    assert ((m == 0.0) | (m > 1e-9 * rk.largest_score(ref))).all()
    # nothing else reaches tau (distance 0 / cosine 1), so the twin alone decides
    np.testing.assert_array_equal(ref["better"], lower.astype(np.int32))
    _load(eng, g, lab)
    better, gen, _ = _rank(eng, q, pl, metric)
    np.testing.assert_array_equal(better, ref["better"])
    np.testing.assert_array_equal(gen["key"] & 0xFFFFFFFF, ref["row_gen"])


@functools.lru_cache(maxsize=None)
def integer_case(n, k):
    """range search's integer recipe (six centres, +-1 noise, components in [-8, 8]: every fp32
    partial sum is an exact integer) with 12 identities dealt independently of the centres, so
    that other identities' best scores land exactly on, one below and one above tau."""
    rng = np.random.default_rng(n + k)
    centres = rng.integers(-7, 8, (6, k))
    x = np.clip(centres[rng.integers(0, 6, n + 50)] + rng.integers(-1, 2, (n + 50, k)), -8, 8).astype(np.float32)
    lab_all = rng.integers(0, 12, n + 50).astype(np.int32) * 3 - 9
    g, q, lab, pl = x[:n], x[n:], lab_all[:n], lab_all[n:]
    ref = rk.reference(q, g, lab, pl, "l2", gram=True)
    s = ref["scores"]
    assert (s == np.rint(s)).all() and s.max() < 2 ** 23
    diff = ref["best"] - ref["tau"][:, None]
    diff = diff[np.isfinite(diff)]
    assert (diff == 0).sum() >= 5 and (diff == -1).sum() >= 5 and (diff == 1).sum() >= 5
    assert (ref["better"] >= 0).all() and np.unique(ref["better"]).size >= 4
    _freeze(g, q, lab, pl)
    return g, lab, q, pl, ref


@pytest.mark.parametrize("n,k", ((300, 20), (200, 130)))
def test_integer_scores_on_the_threshold(eng, n, k):
    """An other-identity score equal to tau beats the genuine row from a lower row only; tau - 1
    always does, tau + 1 never."""
    g, lab, q, pl, ref = integer_case(n, k)
    _check(eng, g, lab, q, pl, "l2", ref)


# ------------------------------------------------------------------ 4. leave-one-out
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_leave_one_out(eng, metric):
    g, lab, _, _, _, _ = blob_case(300, 100, 33, metric)
    rows = np.arange(300, dtype=np.int64)
    ref = rk.reference(g, g, lab, lab, metric, rows)
    rk.clear_margins(ref)
    assert (ref["row_gen"] != rows).all() and (ref["better"] >= 0).all()
    better, _, _ = _check(eng, g, lab, g, lab, metric, ref, rows)
    # rank 1 is what the labelled search calls correct, wherever fp32 keys can tell the two apart
    gk = eng.search_labelled_keys(g, lab, "same", rows, metric)
    ik = eng.search_labelled_keys(g, lab, "other", rows, metric)
    clear = ref["margin"] > 1e-5 * rk.largest_score(ref)
    assert clear.mean() > 0.9
    np.testing.assert_array_equal((better == 0)[clear], (gk < ik)[clear])
    assert 0 < (better == 0).sum() < 300
    again = ev.identification_ranks(g, lab, metric, batch=64, engine=eng)
    assert again.dtype == np.int32 and again.tobytes() == better.tobytes()
    r, c = ev.cmc_curve(better)
    assert c[0] == (better == 0).mean() and c[-1] == 1.0


# ------------------------------------------------------------------ 5. pieces
@pytest.mark.parametrize("b,pieces", ((300, 2), (600, 3)))
def test_pieces_do_not_change_the_result(eng, b, pieces):
    g, lab, centres, names = rk.blobs(700, 130, 33, 9)
    rng = np.random.default_rng(b)
    ident = rng.integers(0, 33, b)
    q = (centres[ident] + rng.standard_normal((b, 130))).astype(np.float32)
    pl = names[ident]
    excl = rng.integers(-1, 700, b).astype(np.int64)
    _load(eng, g, lab)
    assert eng.get_option("rank_bitmap_bytes") == DEFAULT_BUDGET
    whole = _rank(eng, q, pl, "l2", excl)
    assert whole[2][1] == 1 == ev.search_rank_plan(b, 700, 33)[2]
    try:
        eng.set_option("rank_bitmap_bytes", 2048)  # two words per probe: one 256-probe block
        assert ev.search_rank_plan(b, 700, 33, 2048) == (2, 256, pieces)
        cut = _rank(eng, q, pl, "l2", excl)
        eng.set_option("rank_bitmap_bytes", 1)
        one = _rank(eng, q, pl, "l2", excl)
    finally:
        eng.set_option("rank_bitmap_bytes", DEFAULT_BUDGET)
    for got in (cut, one):
        assert got[2][1] == pieces
        assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes()
        assert got[2][0] == whole[2][0] and got[2][2] == whole[2][2] == 33
    ref = rk.reference(q, g, lab, pl, "l2", excl)
    rk.clear_margins(ref)
    np.testing.assert_array_equal(whole[0], ref["better"])
    assert np.unique(whole[0]).size >= 8
    with pytest.raises(N.EigenfaceError):
        eng.set_option("rank_bitmap_bytes", 0)


# ------------------------------------------------------------------ work items of several tiles
@functools.lru_cache(maxsize=None)
def lattice_case(k):
    """The range search's lattice (4229 integer rows, 34 tiles with 5 rows in the last; every score
    an exact integer) with 37 identities dealt by row number, and 8192 probes, each a copy of a
    random row under that row's label: a third unchanged, a third with coordinate 6 flipped, a third
    moved by +2 in coordinate 0.  The rows of a lattice group tie at 0, 1 or 2 across identities."""
    n, b = 4229, 8192
    g = cu.lattice(n, k, 7 * k)
    lab = ((np.arange(n) % 37) * 101 - 1500).astype(np.int32)
    rng = np.random.default_rng(2000 + k)
    src = rng.integers(0, n, b)
    q = g[src].copy()
    kind = np.arange(b) % 3
    rng.shuffle(kind)
    q[kind == 1, 6] = 1 - q[kind == 1, 6]
    q[kind == 2, 0] += 2
    pl = lab[src]
    better, row_gen, beating = rk.better_blocked(q, g, lab, pl, "l2", gram=True)
    assert (better >= 0).all() and np.unique(better).size >= 3 and (better == 0).any()
    # beating rows in every tile, in both tiles of a two-tile item, in the 5-row tail
    tiles = np.flatnonzero(beating) // 128
    assert np.unique(tiles).size == 34 and (tiles % 2 == 1).sum() > 100 and (tiles == 33).any()
    # a class id taken from the tile before or after is another class
    assert (lab[:-128] != lab[128:]).all()
    _freeze(g, lab, q, pl, better, row_gen)
    return g, lab, q, pl, better, row_gen


@pytest.mark.parametrize("k", (16, 40))
def test_work_items_of_several_tiles(eng, k):
    """The planner's branch of two row tiles per item (the range search's own case): the class ids
    of an item's second tile sit in the odd LDS slot.  k = 16 is one slice per tile, k = 40 four."""
    from eigenface import neighbors as nb
    assert nb.search_range_plan(8192, 4229, cu.kp_of(k)) == (17, 2)
    g, lab, q, pl, want, row_gen = lattice_case(k)
    _load(eng, g, lab)
    better, gen, info = _rank(eng, q, pl, "l2")
    np.testing.assert_array_equal(better, want)
    np.testing.assert_array_equal(gen["key"] & 0xFFFFFFFF, row_gen)
    assert info[2] == 37 and info[1] == 1 and info[0] >= 8192


# ------------------------------------------------------------------ 6. given thresholds, additivity
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_shards_by_identity_add_up(eng, metric):
    g0, lab0, centres, names = rk.blobs(400, 40, 20, 21)
    first = np.isin(lab0, names[:9])  # nine identities on shard A, eleven on shard B
    order = np.concatenate([np.flatnonzero(first), np.flatnonzero(~first)])
    g, lab = g0[order], lab0[order]
    na = int(first.sum())
    rng = np.random.default_rng(22)
    ident = rng.integers(0, 20, 90)
    q = (centres[ident] + rng.standard_normal((90, 40))).astype(np.float32)
    pl = names[ident].copy()
    pl[7] = 31337  # nobody's label: -1 on every shard
    excl = rng.integers(-1, 400, 90).astype(np.int64)  # global rows
    ref = rk.reference(q, g, lab, pl, metric, excl)
    rk.clear_margins(ref)
    _load(eng, g, lab)
    whole, gen_whole, _ = _rank(eng, q, pl, metric, excl)
    np.testing.assert_array_equal(whole, ref["better"])
    assert whole[7] == -1 and (np.delete(whole, 7) >= 0).all()
    parts = np.empty(2 * 90, N.MATCH_DTYPE)
    shards = ((g[:na], lab[:na], 0), (g[na:], lab[na:], na))
    for i, (gs, ls, off) in enumerate(shards):
        _load(eng, gs, ls, off)
        parts[90 * i:90 * (i + 1)] = eng.search_labelled_matches(q, pl, "same", excl, metric)
    merged, keys = np.empty(90, N.MATCH_DTYPE), np.empty(90, np.int64)
    assert N.lib().ef_matches_merge(None, parts.ctypes.data, 2, 90, keys.ctypes.data, merged.ctypes.data, 0) == N.EF_OK
    np.testing.assert_array_equal(merged["key"], gen_whole["key"])
    total = np.zeros(90, np.int64)
    for gs, ls, off in shards:
        _load(eng, gs, ls, off)
        part, gen, info = _rank(eng, q, pl, metric, excl, genuine=merged)
        assert gen.tobytes() == merged.tobytes()  # an input: handed back untouched
        shard_ref = rk.reference(q, gs, ls, pl, metric, excl, offset=off,
                                 genuine=(ref["row_gen"], ref["tau"]))
        np.testing.assert_array_equal(part, shard_ref["better"])
        assert part[7] == -1 and (np.delete(part, 7) >= 0).all()
        total += part
    total[7] = -1
    np.testing.assert_array_equal(total, whole)
    _load(eng, g, lab)
    again, _, _ = _rank(eng, q, pl, metric, excl, genuine=gen_whole)  # given its own records: the same
    assert again.tobytes() == whole.tobytes()


# ------------------------------------------------------------------ 7. non-finite and degenerate
@functools.lru_cache(maxsize=None)
def odd_case(metric):
    g, lab, centres, names = rk.blobs(300, 20, 15, 41)
    g = g.copy()
    rng = np.random.default_rng(42)
    ident = rng.integers(0, 15, 40)
    q = (centres[ident] + rng.standard_normal((40, 20))).astype(np.float32)
    pl = names[ident]
    g[5, 3] = np.nan
    g[9, 0] = np.inf
    g[200] = 0.0
    q[4, 7] = np.nan
    q[6] = 0.0
    ref = rk.reference(q, g, lab, pl, metric)
    rk.clear_margins(ref, exact=(6,) if metric == "cosine" else ())
    assert not ref["ok"][:, [5, 9]].any() and ref["better"][4] == -1
    assert (np.delete(ref["better"], 4) >= 0).all()
    if metric == "cosine":  # the zero probe scores 0 everywhere: the first row of its label is genuine
        first = int(np.flatnonzero((lab == pl[6]) & np.isfinite(g).all(axis=1))[0])
        assert ref["row_gen"][6] == first and ref["better"][6] == np.unique(lab[:first][np.isfinite(g[:first]).all(axis=1)]).size
    _freeze(g, lab, q, pl)
    return g, lab, q, pl, ref


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_non_finite_rows_and_probes(eng, metric):
    g, lab, q, pl, ref = odd_case(metric)
    _load(eng, g, lab)
    better, gen, info = _rank(eng, q, pl, metric)
    np.testing.assert_array_equal(better, ref["better"])
    assert gen["key"][4] == N.EF_KEY_NONE
    twice = _rank(eng, q, pl, metric)
    for x, y in zip((better, gen, info), twice):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_device_tensors_on_a_callers_stream(eng, metric):
    import torch
    g, lab, q, pl, ref, _ = blob_case(700, 130, 65, metric)
    host = _check(eng, g, lab, q, pl, metric, ref)
    stream = torch.cuda.Stream()
    outs = []
    with torch.cuda.stream(stream):
        qd = torch.as_tensor(q.copy(), device="cuda")
        pd = torch.as_tensor(pl.copy(), device="cuda")
        mine = torch.full((77,), -5, dtype=torch.int32, device="cuda")
        outs.append(eng.search_rank(qd, pd, None, metric))
        outs.append(eng.search_rank(qd, pd, None, metric, out=mine))
        assert outs[1][0] is mine
        outs.append(eng.search_rank(qd, pd, None, metric, genuine=outs[0][1]))
    stream.synchronize()
    for better, gen, info in outs:
        assert better.is_cuda and gen.is_cuda and info.is_cuda
        assert better.dtype == torch.int32 and tuple(gen.shape) == (77, 3) and gen.dtype == torch.int64
        for x, y in zip((better, gen, info), host):
            assert x.cpu().numpy().tobytes() == y.tobytes()  # byte-equal to the host call, and run to run


def test_new_labels_rebuild_the_class_map(eng):
    g, lab, q, pl, ref, _ = blob_case(300, 100, 33, "l2")
    _load(eng, g, lab)
    np.testing.assert_array_equal(_rank(eng, q, pl, "l2")[0], ref["better"])
    names = np.unique(lab)
    merged = {int(v): int(names[i // 3 * 3]) for i, v in enumerate(names)}  # three identities become one
    lab2 = np.array([merged[int(v)] for v in lab], np.int32)
    pl2 = np.array([merged[int(v)] for v in pl], np.int32)
    ref2 = rk.reference(q, g, lab2, pl2, "l2")
    rk.clear_margins(ref2)
    assert not np.array_equal(ref2["better"], ref["better"])
    eng.set_gallery_labels(lab2)
    better, _, info = _rank(eng, q, pl2, "l2")
    np.testing.assert_array_equal(better, ref2["better"])
    assert info[2] == 11
    eng.set_gallery(g)  # a new gallery drops the labels, and the map with them
    with pytest.raises(N.EigenfaceError):
        eng.search_rank(q, pl2)
    eng.set_gallery_labels(lab)
    np.testing.assert_array_equal(_rank(eng, q, pl, "l2")[0], ref["better"])


def test_state_and_arguments(eng):
    from eigenface import Engine
    lib = N.lib()
    rng = np.random.default_rng(2)
    q = rng.standard_normal((4, 5)).astype(np.float32)
    pl = np.array([1, 2, 1, 3], np.int32)
    better, info = np.zeros(4, np.int32), np.zeros(4, np.int64)
    gen = np.zeros(4, N.MATCH_DTYPE)

    def call(h, qp=q.ctypes.data, b=4, metric=N.EF_METRIC_L2, lp=pl.ctypes.data, gp=gen.ctypes.data,
             bp=better.ctypes.data, ip=info.ctypes.data, flags=0):
        return lib.ef_search_rank(h, qp, b, metric, lp, None, gp, bp, ip, flags)
    g = rng.standard_normal((8, 5)).astype(np.float32)
    lab = np.array([1, 1, 2, 2, 3, 3, 4, 4], np.int32)
    with Engine(0) as fresh:
        with pytest.raises(RuntimeError):
            fresh.search_rank(q, pl)
        assert call(fresh._h) == N.EF_E_STATE  # no gallery
        fresh.set_gallery(g)
        assert call(fresh._h) == N.EF_E_STATE  # no labels
        with pytest.raises(N.EigenfaceError):
            fresh.search_rank(q, pl)
        # an empty gallery: EF_OK, nobody has a genuine row, info all zero
        fresh.set_gallery(np.zeros((0, 5), np.float32))
        fresh.set_gallery_labels(np.zeros(0, np.int32))
        better[:], info[:] = 7, -1
        assert call(fresh._h) == N.EF_OK and (better == -1).all() and (info == 0).all()
        assert (gen["key"] == N.EF_KEY_NONE).all()
        b0, g0, i0 = fresh.search_rank(q, pl)
        assert (b0 == -1).all() and (i0 == 0).all() and (g0["key"] == N.EF_KEY_NONE).all()
    _load(eng, g, lab)
    assert call(eng._h, metric=7) == N.EF_E_INVALID
    assert call(eng._h, lp=None) == N.EF_E_INVALID
    assert call(eng._h, bp=None) == N.EF_E_INVALID
    assert call(eng._h, ip=None) == N.EF_E_INVALID
    assert call(eng._h, qp=None) == N.EF_E_INVALID
    assert call(eng._h, b=-1) == N.EF_E_INVALID
    assert call(eng._h, gp=None, flags=N.EF_RANK_GENUINE_GIVEN) == N.EF_E_INVALID
    assert call(eng._h) == N.EF_OK
    assert call(eng._h, gp=None) == N.EF_OK  # the records are optional
    ref = rk.reference(q, g, lab, pl, "l2")
    np.testing.assert_array_equal(better, ref["better"])
    better[:], info[:] = 7, -1
    assert call(eng._h, b=0) == N.EF_OK and (better == 7).all()  # b = 0 writes no probe's entry
    b0, g0, i0 = eng.search_rank(q[:0], pl[:0])
    assert b0.shape == (0,) and g0.shape == (0,)
    with pytest.raises(ValueError):
        eng.search_rank(q, None)
    with pytest.raises(ValueError):
        eng.search_rank(q, pl[:3])
    with pytest.raises(ValueError):
        eng.search_rank(q[:, :4], pl)
    with pytest.raises(ValueError):
        eng.search_rank(q, pl, exclude_rows=np.zeros(3, np.int64))
    with pytest.raises(ValueError):
        eng.search_rank(q, pl, out=better)  # out is for device input
    with pytest.raises(ValueError):
        eng.search_rank(q, pl, genuine=gen[:3])
    # the timer covers the call
    eng.timing(True)
    eng.timing_reset()
    eng.search_rank(q, pl)
    ms, launches = eng.timing_get("rank")
    eng.timing(False)
    assert launches == 1 and ms > 0.0


def test_recognize_rank_projects_first(eng):
    rng = np.random.default_rng(5)
    d, k, n = 96, 12, 150
    mean = rng.standard_normal(d).astype(np.float32)
    W = (rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32)
    eng.set_model(mean, W)
    P = rng.standard_normal((n + 30, d)).astype(np.float32) * 3
    f = eng.project(P)
    lab = (np.arange(n) % 10).astype(np.int32)
    pl = (np.arange(30) % 10).astype(np.int32)
    _load(eng, f[:n], lab)
    a = eng.recognize_rank(P[n:], pl, metric="cosine")
    b = eng.search_rank(f[n:], pl, metric="cosine")
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert np.unique(a[0]).size >= 4


# ------------------------------------------------------------------ 8. outside the scan's domain
def test_a_huge_probe_is_settled_in_fp64(eng):
    """Cosine: a probe of norm ~1e37 has max|g| |q| beyond 2^126, so delta_p = +inf: each of its
    pairs with a finite scan score is settled in fp64, the neighbours' are not."""
    g, lab, q, pl, ref, _ = blob_case(300, 100, 33, "cosine")
    huge = (q[3].astype(np.float64) * 1e36).astype(np.float32)
    gm = np.sqrt((g.astype(np.float64) ** 2).sum(axis=1).max())
    qn = np.linalg.norm(huge.astype(np.float64))
    assert np.isfinite(huge).all() and gm * gm + 2.02 * gm * qn > 2.0 ** 126 and gm * qn < 3e38
    q2 = np.concatenate([q, huge[None, :]])
    pl2 = np.concatenate([pl, pl[3:4]])
    ref2 = rk.reference(q2, g, lab, pl2, "cosine")
    rk.clear_margins(ref2)
    assert ref2["better"][-1] == ref2["better"][3]  # cosine does not see the scale
    _load(eng, g, lab)
    base = _rank(eng, q, pl, "cosine")
    np.testing.assert_array_equal(base[0], ref2["better"][:-1])
    better, _, info = _rank(eng, q2, pl2, "cosine")
    np.testing.assert_array_equal(better, ref2["better"])
    assert info[0] - base[2][0] == 300  # every pair of the huge probe, nothing more
