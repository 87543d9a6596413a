"""Score census (ef_score_census): the genuine and impostor score histograms of a labelled
gallery against fp64 references.  Exact counts where every fp32 partial sum is an integer, the
guarantee's cumulative bracket on real-valued features (delta from the formula in
include/eigenface.h, never from the kernel's output), and the analytic count where every pair
lands in one bin.  Every input condition is asserted on the reference first."""
import ctypes
import functools

import numpy as np
import pytest

import labelled_util as lu

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NCLS = 6
ABSENT = 3  # a probe label no gallery row carries


def _kp(k):  # csrc/ef_internal.hpp feature_pad
    for p in (16, 32, 64, 128, 256, 512):
        if k <= p:
            return p
    return (k + 127) // 128 * 128


def _labels(rng, n, b):
    """Unsorted labels; class ABSENT is in no gallery, and some probes carry it."""
    pool = np.array([c for c in range(NCLS) if c != ABSENT], np.int32)
    glab = pool[rng.integers(0, len(pool), n)]
    plab = rng.integers(0, NCLS, b).astype(np.int32)
    plab[:3] = (ABSENT, pool[0], ABSENT)[:min(3, b)]
    return glab, plab


def _excl(rng, n, b):
    """A mix of valid rows, 'none' (negative) and rows outside the gallery."""
    e = rng.integers(0, n, b).astype(np.int64)
    e[1::3] = -1
    e[2::3] = n + 5
    return e


@functools.lru_cache(maxsize=None)
def integer_case(k, n, b):
    """Integers in [-8, 8]: class centres plus noise in {-1, 0, 1}, clipped, so that genuine
    squared distances stay inside 2048 unit bins while every fp32 partial sum is an integer
    below 2^24 (k * 16^2 <= 163840)."""
    rng = np.random.default_rng(1000 * k + n + b)
    centres = rng.integers(-8, 9, (NCLS, k))
    glab, plab = _labels(rng, n, b)
    g = np.clip(centres[glab] + rng.integers(-1, 2, (n, k)), -8, 8).astype(np.float32)
    q = np.clip(centres[plab] + rng.integers(-1, 2, (b, k)), -8, 8).astype(np.float32)
    excl = _excl(rng, n, b)
    for a in (g, q, glab, plab, excl):
        a.setflags(write=False)
    return g, q, glab, plab, excl


def _sides(glab, plab, excl, n):
    return lu.qualifies(glab, plab, "same", excl, n), lu.qualifies(glab, plab, "other", excl, n)


def _slots(s, lo, hi, nbins):
    """fp64 slot of every score: 0 below lo, 1 + bin, nbins + 1 from hi on."""
    j = np.floor((np.asarray(s, np.float64) - lo) * nbins / (hi - lo)) + 1
    return np.clip(j, 0, nbins + 1).astype(np.int64)


def _reference(s, masks, lo, hi, nbins, finite=None):
    """counts[2][nbins + 3] by np.histogram on the fp64 scores of each side; pairs outside
    ``finite`` go to the last slot."""
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    out = np.zeros((2, nbins + 3), np.int64)
    for side, m in enumerate(masks):
        ok = m if finite is None else m & finite
        v = s[ok]
        out[side, 0] = (v < lo).sum()
        out[side, 1:nbins + 1] = np.histogram(v[(v >= lo) & (v < hi)], bins=edges)[0]
        out[side, nbins + 1] = (v >= hi).sum()
        out[side, nbins + 2] = m.sum() - ok.sum()
    return out


def _integer_bins(s):
    # 2048 unit bins where the largest score allows it, else fewer, so that mass falls in the over slot
    return 2048 if s.max() < 2047 else 1000


@functools.lru_cache(maxsize=None)
def integer_ref(k, n, b):
    g, q, glab, plab, excl = integer_case(k, n, b)
    s = lu.score_matrix(q, g, "l2")
    assert (s == np.rint(s)).all() and s.max() < 2 ** 23
    nbins = _integer_bins(s)
    ref = _reference(s, _sides(glab, plab, excl, n), -0.5, -0.5 + nbins, nbins)
    ref.setflags(write=False)
    return ref, nbins


def _load(eng, g, glab, offset=0):
    eng.set_gallery(g, global_offset=offset)
    eng.set_gallery_labels(glab)


INTEGER_CASES = ((8, 1, 1), (20, 63, 33), (16, 64, 257), (128, 65, 256), (128, 200, 513), (160, 5003, 257),
                 (640, 200, 33))


# ------------------------------------------------- 1. exact counts on representable scores
@pytest.mark.parametrize("k,n,b", INTEGER_CASES)
def test_exact_counts(eng, k, n, b):
    g, q, glab, plab, excl = integer_case(k, n, b)
    ref, nbins = integer_ref(k, n, b)
    if n >= 63:  # input conditions: both sides populated, an absent class, every kind of exclusion
        assert ref[0].sum() > 0 and ref[1].sum() > 0 and (plab == ABSENT).any() and not (glab == ABSENT).any()
        assert (excl < 0).any() and (excl >= n).any() and ((excl >= 0) & (excl < n)).any()
    if nbins < 2048:
        assert ref[:, nbins + 1].sum() > 0  # mass in the over slot
    _load(eng, g, glab)
    got = eng.score_census(q, plab, excl, "l2", nbins, (-0.5, -0.5 + nbins))
    assert got.dtype == np.int64 and got.shape == (2, nbins + 3)
    np.testing.assert_array_equal(got, ref)
    # deterministic: integer accumulation only
    np.testing.assert_array_equal(eng.score_census(q, plab, excl, "l2", nbins, (-0.5, -0.5 + nbins)), got)


# --------------------------------------------- 2. bracketed counts on real-valued features
@functools.lru_cache(maxsize=None)
def real_case(k, n):
    """Clustered normal features: class centres plus 0.5 sigma noise."""
    rng = np.random.default_rng(77 * k + n)
    centres = rng.standard_normal((NCLS, k))
    glab = rng.integers(0, NCLS, n).astype(np.int32)
    g = (centres[glab] + 0.5 * rng.standard_normal((n, k))).astype(np.float32)
    g.setflags(write=False)
    glab.setflags(write=False)
    return g, glab


@functools.lru_cache(maxsize=None)
def real_scores(k, n, b, metric):
    g, _ = real_case(k, n)
    s = lu.score_matrix(g[:b], g, metric)
    s = s if metric == "l2" else -s  # the user-facing similarity
    s.setflags(write=False)
    return s


def _delta(k, q, g, s, lo, hi, metric):
    """The guarantee's delta (include/eigenface.h, ef_score_census)."""
    kp = _kp(k)
    edge = 8 * U * max(abs(lo), abs(hi))
    if metric == "cosine":
        return 2 * (kp + 12) * U * 1.01 + edge
    qn = np.sqrt((np.asarray(q, np.float64) ** 2).sum(1).max())
    gn = np.sqrt((np.asarray(g, np.float64) ** 2).sum(1).max())
    return 2 * ((kp + 4) * U * 1.01 * (2 * qn * gn + gn * gn) + 4 * U * np.abs(s).max()) + edge


def _real_range(s, metric, nbins, self_pairs=True):
    """float32 (lo, hi).  L2: lo one bin width below 0; the top of the scores falls in the over
    slot.  That puts the edge lo + w on 0 itself, so where the probes' own rows are counted
    (``self_pairs``: b pairs at distance 0, 3 % of the genuine side at n = 203) lo is HALF a bin
    width below 0 instead, and no edge sits on the self-distance.  Cosine: a range past +-1, so
    that no edge sits on the self-similarity 1."""
    if metric == "cosine":
        return -1.0625, 1.0625
    w = float(s.max()) / nbins
    below = w / 2 if self_pairs else w
    return float(np.float32(-below)), float(np.float32(nbins * w - below))


def _assert_bracket(got, s, masks, lo, hi, nbins, delta):
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    for side, m in enumerate(masks):
        v = np.sort(s[m])
        near = np.zeros(v.shape, bool)
        for e in edges:
            near |= np.abs(v - e) <= delta
        assert near.mean() <= 0.02 if v.size else True, f"side {side}: {near.mean():.4f} of the pairs within delta of an edge"
        assert got[side].sum() == v.size and got[side, nbins + 2] == 0
        below = np.cumsum(got[side])[:nbins + 1]  # binned below edge j: slots 0 .. j
        lower = np.searchsorted(v, edges - delta, side="left")   # score < e - delta
        upper = np.searchsorted(v, edges + delta, side="left")   # score < e + delta
        bad = (below < lower) | (below > upper)
        assert not bad.any(), f"side {side}: edges {np.flatnonzero(bad)[:5]} outside the bracket: " \
                              f"{below[bad][:5]} not in [{lower[bad][:5]}, {upper[bad][:5]}]"


@pytest.mark.parametrize("metric", ("l2", "cosine"))
@pytest.mark.parametrize("k,n,b", ((16, 1000, 257), (128, 1000, 257), (20, 203, 33), (640, 203, 33)))
def test_bracketed_counts(eng, k, n, b, metric):
    g, glab = real_case(k, n)
    q, plab = g[:b], glab[:b]  # the probes are gallery rows
    s = real_scores(k, n, b, metric)
    _load(eng, g, glab)
    for own_excluded in (True, False):
        excl = np.arange(b, dtype=np.int64) if own_excluded else None
        masks = _sides(glab, plab, excl, n)
        for nbins in (1, 7, 64):
            lo, hi = _real_range(s, metric, nbins, self_pairs=not own_excluded)
            delta = _delta(k, q, g, s, lo, hi, metric)
            got = eng.score_census(q, plab, excl, metric, nbins, (lo, hi))
            _assert_bracket(got, s, masks, lo, hi, nbins, delta)


# ------------------------------------------- 2b. work items ("chunks") of several tiles
# Every case above runs one gallery tile per work item, and test_one_bin_past_32_bits, which does
# not, repeats one row and labels i % 2, so all its tiles are alike.  Here the planner gives two
# tiles per item, the last item ends on a 5-row tile, and rows, norms and labels differ from tile
# to tile.  The references are built over blocks of probes: no b x n array is held.
CHUNK_N, CHUNK_B = 4229, 8192


def _assert_chunk_plan(n, b):
    """launch_census's plan restated: tiles per work item, and where the ragged tile falls."""
    n_ptiles = (b + 127) // 128
    tiles = (n + 127) // 128
    want = max(1, (2048 + n_ptiles - 1) // n_ptiles)
    tpc = (tiles + min(want, tiles) - 1) // min(want, tiles)
    assert tiles > want and tpc >= 2
    assert n % 128 != 0 and (tiles - 1) % tpc != 0  # the ragged last tile is a later tile of its item
    return tpc


def _assert_tiles_differ(g, glab):
    """A value taken from the tile before or after is another value, for labels and norms alike."""
    sq = (np.asarray(g, np.float64) ** 2).sum(1)
    assert (glab[:-128] != glab[128:]).mean() > 0.5
    assert (sq[:-128] != sq[128:]).mean() > 0.9
    with np.errstate(divide="raise"):
        assert (1 / np.sqrt(sq[:-128]) != 1 / np.sqrt(sq[128:])).mean() > 0.9


@functools.lru_cache(maxsize=None)
def chunk_integer_ref(k):
    """counts[2][nbins + 3] by np.bincount on the exact integer scores, 512 probes at a time."""
    n, b = CHUNK_N, CHUNK_B
    g, q, glab, plab, excl = integer_case(k, n, b)
    top, per_block = 0, []
    for a in range(0, b, 512):
        s = lu.score_matrix(q[a:a + 512], g, "l2")
        si = np.rint(s).astype(np.int64)
        assert (s == si).all() and si.min() >= 0 and si.max() < 2 ** 23  # every fp32 partial sum is an exact integer
        top = max(top, int(si.max()))
        per_block.append((si, _sides(glab, plab[a:a + 512], excl[a:a + 512], n)))
    # 2048 bins from -0.5 on, of the smallest width 2^j that holds every score: the edges are
    # half-integers, no score lies on one, and (score + 0.5) / width is exact in fp32
    nbins, width = 2048, 1
    while top >= nbins * width:
        width *= 2
    ref = np.zeros((2, nbins + 3), np.int64)
    for si, masks in per_block:
        slot = si // width + 1
        for side, m in enumerate(masks):
            ref[side] += np.bincount(slot[m], minlength=nbins + 3)
    ref.setflags(write=False)
    return ref, nbins, width


@pytest.mark.parametrize("k", (16, 40))
def test_chunks_of_several_tiles(eng, k):
    n, b = CHUNK_N, CHUNK_B
    assert _assert_chunk_plan(n, b) == 2 and n - 33 * 128 == 5 and _kp(k) // 16 == (1 if k == 16 else 4)
    g, q, glab, plab, excl = integer_case(k, n, b)
    _assert_tiles_differ(g, glab)
    assert (plab == ABSENT).any() and not (glab == ABSENT).any()
    assert (excl < 0).any() and (excl >= n).any() and ((excl >= 0) & (excl < n)).any()
    ref, nbins, width = chunk_integer_ref(k)
    assert ref.sum() == b * n - ((excl >= 0) & (excl < n)).sum()
    assert ((ref[:, 1:nbins + 1] > 0).sum(axis=1) > 40).all()  # both sides spread over many bins
    rng_ = (-0.5, -0.5 + nbins * width)
    _load(eng, g, glab)
    got = eng.score_census(q, plab, excl, "l2", nbins, rng_)
    assert got.dtype == np.int64 and got.shape == (2, nbins + 3)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(eng.score_census(q, plab, excl, "l2", nbins, rng_), got)


def _bracket_bounds(blocks, lo, hi, nbins, delta):
    """_assert_bracket's reference side over blocks of (scores, (genuine mask, impostor mask)):
    per side the number of pairs, of pairs within delta of an edge, and per edge the pairs below
    edge - delta and below edge + delta."""
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    assert 2 * delta < (hi - lo) / nbins  # the intervals around the edges are disjoint
    marks = np.stack([edges - delta, edges + delta], axis=1).ravel()  # ascending
    assert (np.diff(marks) > 0).all()
    size, near, below = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros((2, marks.size + 1), np.int64)
    for s, masks in blocks:
        for side, m in enumerate(masks):
            v = s[m]
            c = np.searchsorted(marks, v, side="right")  # marks at or below the score
            size[side] += v.size
            below[side] += np.bincount(c, minlength=marks.size + 1)
            # |v - e| <= delta: from e - delta on (c odd) or on e + delta itself
            near[side] += ((c % 2 == 1) | (v == marks[np.maximum(c, 1) - 1])).sum()
    cum = np.cumsum(below, axis=1)[:, :-1]  # pairs with score < marks[i] (c <= i)
    return size, near, cum[:, 0::2], cum[:, 1::2]


def _assert_bracket_bounds(got, bounds, nbins):
    size, near, lower, upper = bounds
    for side in range(2):
        assert got[side].sum() == size[side] and got[side, nbins + 2] == 0
        below = np.cumsum(got[side])[:nbins + 1]  # binned below edge j: slots 0 .. j
        bad = (below < lower[side]) | (below > upper[side])
        assert not bad.any(), f"side {side}: edges {np.flatnonzero(bad)[:5]} outside the bracket: " \
                              f"{below[bad][:5]} not in [{lower[side][bad][:5]}, {upper[side][bad][:5]}]"


def test_bracket_bounds_equal_assert_brackets_own():
    """The blockwise bounds are _assert_bracket's: equal on a case small enough for both."""
    k, n, b, nbins = 16, 1000, 257, 64
    g, glab = real_case(k, n)
    s = real_scores(k, n, b, "cosine")
    masks = _sides(glab, glab[:b], None, n)
    lo, hi = _real_range(s, "cosine", nbins)
    delta = 1e-3  # wide enough that pairs fall within it
    blocks = [(s[a:a + 100], tuple(m[a:a + 100] for m in masks)) for a in range(0, b, 100)]
    size, near, lower, upper = _bracket_bounds(blocks, lo, hi, nbins, delta)
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    for side, m in enumerate(masks):
        v = np.sort(s[m])
        want_near = np.zeros(v.shape, bool)
        for e in edges:
            want_near |= np.abs(v - e) <= delta
        assert size[side] == v.size and near[side] == want_near.sum() > 0
        np.testing.assert_array_equal(lower[side], np.searchsorted(v, edges - delta, side="left"))
        np.testing.assert_array_equal(upper[side], np.searchsorted(v, edges + delta, side="left"))


def test_chunks_of_several_tiles_cosine(eng):
    """The same plan on real-valued features under cosine, where the rows' 1 / |g| are read from
    the aux slot in the epilogue: the guarantee's bracket, its bounds built block by block."""
    k, n, b, nbins = 16, CHUNK_N, CHUNK_B, 64
    assert _assert_chunk_plan(n, b) == 2
    feats, labs = real_case(k, n + b)  # one set of class centres: the gallery, then the probes
    g, glab, q, plab = feats[:n], labs[:n], feats[n:], labs[n:]
    _assert_tiles_differ(g, glab)
    excl = _excl(np.random.default_rng(k + n + b), n, b)
    lo, hi = -1.0625, 1.0625
    delta = _delta(k, q, g, None, lo, hi, "cosine")
    blocks = ((-lu.score_matrix(q[a:a + 512], g, "cosine"), _sides(glab, plab[a:a + 512], excl[a:a + 512], n))
              for a in range(0, b, 512))
    bounds = _bracket_bounds(blocks, lo, hi, nbins, delta)
    size, near = bounds[:2]
    assert (size > 0).all() and size.sum() == b * n - ((excl >= 0) & (excl < n)).sum()
    assert (near <= 0.02 * size).all(), near / size  # _assert_bracket's cap, before the GPU is asked
    assert ((bounds[3] - bounds[2]).max(axis=1) > 0).all() or near.sum() == 0
    _load(eng, g, glab)
    got = eng.score_census(q, plab, excl, "cosine", nbins, (lo, hi))
    _assert_bracket_bounds(got, bounds, nbins)
    np.testing.assert_array_equal(eng.score_census(q, plab, excl, "cosine", nbins, (lo, hi)), got)


# ------------------------------------------------ 3. contention and 64-bit accumulation
def _one_vector(eng, k, n, b, metric, nbins, rng_, slot, excl):
    v = np.arange(1, k + 1, dtype=np.float32) % 5 - 2  # small integers: every sum is exact
    v[0] = 1
    g = np.broadcast_to(v, (n, k)).copy()
    q = np.broadcast_to(v, (b, k)).copy()
    glab = (np.arange(n) % 2).astype(np.int32)  # half the rows carry the probes' label 1
    plab = np.ones(b, np.int32)
    _load(eng, g, glab)
    got = eng.score_census(q, plab, excl, metric, nbins, rng_)
    same = int(glab.sum())
    want = np.zeros((2, nbins + 3), np.int64)
    want[0, slot] = b * same
    want[1, slot] = b * (n - same)
    if excl is not None:  # probe p leaves out row p: odd rows are genuine
        want[0, slot] -= int((np.arange(b) % 2 == 1).sum())
        want[1, slot] -= int((np.arange(b) % 2 == 0).sum())
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_one_bin_small(eng, metric):
    # L2: every distance is exactly 0, bin 0 of [-0.5, 63.5); cosine: 1 within a few ulps, the
    # middle one of three bins over (0, 2)
    nbins, rng_, slot = (64, (-0.5, 63.5), 1) if metric == "l2" else (3, (0.0, 2.0), 2)
    _one_vector(eng, 128, 5003, 513, metric, nbins, rng_, slot, np.arange(513, dtype=np.int64))


def test_one_bin_past_32_bits(eng):
    n, b = 1_100_000, 4096
    assert b * n > 2 ** 32 and b * (n // 2) > 2 ** 31  # a 32-bit counter wraps on either side
    _one_vector(eng, 8, n, b, "l2", 64, (-0.5, 63.5), 1, None)


# ------------------------------------------------------------------ 4. non-finite inputs
@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_non_finite_inputs(eng, metric):
    k, n, b = 20, 63, 33
    g0, q0, glab, plab, excl = integer_case(k, n, b)
    g, q = g0.copy(), q0.copy()
    g[5, 3] = np.nan
    q[7, 2] = np.inf
    finite = np.ones((b, n), bool)
    finite[:, 5] = False
    finite[7, :] = False
    masks = _sides(glab, plab, excl, n)
    assert all((m & ~finite).any() for m in masks)  # both sides have non-finite pairs
    _load(eng, g, glab)
    if metric == "l2":
        nbins = integer_ref(k, n, b)[1]
        lo, hi = -0.5, -0.5 + nbins
        ref = _reference(lu.score_matrix(q0, g0, "l2"), masks, lo, hi, nbins, finite)
        np.testing.assert_array_equal(eng.score_census(q, plab, excl, "l2", nbins, (lo, hi)), ref)
    else:
        got = eng.score_census(q, plab, excl, "cosine", 16, (-1.0625, 1.0625))
        for side, m in enumerate(masks):
            assert got[side, 18] == (m & ~finite).sum() and got[side].sum() == m.sum()


# ------------------------------------------------------------------------- 5. sharding
def test_shards_add_up(eng):
    k, n, b = 20, 63, 33
    g, q, glab, plab, excl = integer_case(k, n, b)
    ref, nbins = integer_ref(k, n, b)
    total = np.zeros_like(ref)
    for a, z in ((0, 31), (31, n)):
        _load(eng, g[a:z], glab[a:z], offset=a)
        total += eng.score_census(q, plab, excl, "l2", nbins, (-0.5, -0.5 + nbins))  # global exclude_rows
    np.testing.assert_array_equal(total, ref)


# ---------------------------------------------- 6. cross-check with the labelled search
def test_lowest_bin_holds_the_labelled_search_score(eng):
    k, n, b, nbins = 128, 1000, 257, 64
    g, glab = real_case(k, n)
    s = real_scores(k, n, b, "l2")
    lo, hi = _real_range(s, "l2", nbins)
    _load(eng, g, glab)
    edges = lo + (hi - lo) * np.arange(nbins + 1) / nbins
    for p in (0, 100, 256):
        q, plab, excl = g[p:p + 1], glab[p:p + 1], np.array([p], np.int64)
        delta = _delta(k, q, g, s[p], lo, hi, "l2")
        got = eng.score_census(q, plab, excl, "l2", nbins, (lo, hi))
        for side, rel in enumerate(("same", "other")):
            idx, best = eng.search_labelled(q, plab, rel, excl, "l2")
            assert idx[0] >= 0
            lowest = int(np.flatnonzero(got[side, :nbins + 2])[0])
            want = int(_slots(float(best[0]), lo, hi, nbins))
            slack = 1 if np.abs(edges - float(best[0])).min() <= delta else 0
            assert abs(lowest - want) <= slack, (p, rel, lowest, want)


# ------------------------------------------------- the leave-one-out census of a gallery
def test_gallery_census_and_comparison(eng):
    from eigenface import compare_verification, score_census, verification_rates
    k, n = 20, 203
    g, glab = real_case(k, n)
    same = glab[None, :] == glab[:, None]
    off = ~np.eye(n, dtype=bool)
    for metric in ("cosine", "l2"):
        counts, (lo, hi) = score_census(g, glab, metric, nbins=64, batch=64, engine=eng)  # four batches
        assert counts.dtype == np.int64 and counts.shape == (2, 67)
        # ordered pairs, each row against all the others; the default range holds every score
        assert counts[0].sum() == (same & off).sum() and counts[1].sum() == (~same).sum()
        assert not counts[:, 0].any() and not counts[:, 66].any()
        if metric == "l2":
            assert lo == 0.0 and hi >= 4 * (g.astype(np.float64) ** 2).sum(1).max() and not counts[:, 65].any()
        else:
            assert (lo, hi) == (-1.0, 1.0)
        one = score_census(g, glab, metric, nbins=64, batch=4096, engine=eng)[0]
        np.testing.assert_array_equal(one, counts)  # the batches add up
        # the histograms against the fp64 scores, through the guarantee's bracket
        s = lu.score_matrix(g, g, metric)
        s = s if metric == "l2" else -s
        _assert_bracket(counts, s, (same & off, ~same), lo, hi, 64, _delta(k, g, g, s, lo, hi, metric))
        r = verification_rates(counts, lo, hi, metric)
        assert (r.n_genuine, r.n_impostor) == (int((same & off).sum()), int((~same).sum()))
    out = compare_verification(g, g[:, :8].copy(), glab, "l2", fmr=(1e-2,), nbins=64, engine=eng)
    assert set(out) == {"pca", "fisher"}
    for v in out.values():
        assert 0.5 < v["auc"] <= 1.0 and 0.0 <= v["tar_at_fmr"][1e-2] <= 1.0 and v["nonfinite"] == (0, 0)


# --------------------------------------------------------------- 7. state and arguments
def test_state_and_arguments(eng):
    from eigenface import EigenfaceError, Engine, _native as N
    rng = np.random.default_rng(5)
    g = rng.standard_normal((200, 24)).astype(np.float32)
    q = rng.standard_normal((37, 24)).astype(np.float32)
    glab = rng.integers(0, 4, 200).astype(np.int32)
    plab = rng.integers(0, 4, 37).astype(np.int32)
    counts = np.zeros((2, 19), np.int64)
    lib = eng._lib

    def call(h, nbins=16, lo=-1.0, hi=1.0, labels=plab.ctypes.data, out=counts.ctypes.data, b=37):
        return lib.ef_score_census(h, q.ctypes.data, b, N.EF_METRIC_COSINE, labels, None, lo, hi, nbins, out, 0)

    with Engine(0) as fresh:  # no gallery
        assert call(fresh._h) == N.EF_E_STATE
        with pytest.raises(RuntimeError):
            fresh.score_census(q, plab)
    eng.set_gallery(g)  # no labels
    assert call(eng._h) == N.EF_E_STATE
    with pytest.raises(EigenfaceError) as ei:
        eng.score_census(q, plab)
    assert ei.value.code == N.EF_E_STATE
    eng.set_gallery_labels(glab)
    assert call(eng._h) == N.EF_OK
    for kw in (dict(nbins=0), dict(nbins=2049), dict(lo=1.0, hi=1.0), dict(lo=1.0, hi=-1.0), dict(lo=float("nan")),
               dict(hi=float("nan")), dict(hi=float("inf")), dict(labels=None), dict(out=None), dict(b=-1)):
        assert call(eng._h, **kw) == N.EF_E_INVALID, kw
    for bad in (dict(nbins=0), dict(nbins=2049), dict(range=(1.0, 1.0)), dict(range=(0.0, float("nan")))):
        with pytest.raises(ValueError):
            eng.score_census(q, plab, **bad)
    # b = 0: zeros
    counts[:] = 7
    assert call(eng._h, b=0) == N.EF_OK and not counts.any()
    assert not eng.score_census(np.zeros((0, 24), np.float32), np.zeros(0, np.int32)).any()
    # device tensors in, device counts out: the host-pointer result
    import torch
    host = eng.score_census(q, plab, np.arange(37), "cosine", 16)
    dev = eng.score_census(torch.as_tensor(q).cuda(), torch.as_tensor(plab).cuda(), torch.arange(37).cuda(), "cosine", 16)
    assert dev.is_cuda and dev.dtype == torch.int64
    np.testing.assert_array_equal(dev.cpu().numpy(), host)
    assert host.sum() == 37 * 200 - 37
