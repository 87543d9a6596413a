"""Single-bf16 screen ahead of the split-bf16 prefix scan (EF_OPT_SEARCH_PREFIX_SCREEN, the
default): keys and match records must equal those with the screen off and those
of the plain full-k pipeline bit for bit, the screen must prove with the documented per-row
bound, and its guard and counters must behave as documented."""
import functools

import numpy as np
import pytest

import prefix_screen_util as ps
from eigenface import synth
from eigenface._native import EigenfaceError
from parity_util import assert_exact_argbest

pytestmark = pytest.mark.gpu
EF_E_INVALID = -1  # include/eigenface.h


@pytest.fixture(autouse=True)
def _default_options(eng):
    yield
    eng.set_option("search_prefix", 1)
    eng.set_option("search_prefix_split", 1)
    eng.set_option("search_prefix_screen", 1)


def _search(eng, q, k1, screen, matches=True):
    """(keys, records, search_stats, search_screen_stats) at prefix length k1 (0: the plain
    pipeline) with the screen on or off.  Setting the options clears the guards."""
    eng.set_option("search_prefix_screen", screen)
    eng.set_option("search_prefix", k1)
    keys = eng.search_keys(q)
    st, ss = eng.search_stats(), eng.search_screen_stats()
    m = None
    if matches:
        eng.set_option("search_prefix", k1)
        m = eng.search_matches(q)
    return keys, m, st, ss


def _three_ways(eng, g, q, k1, offset=0, matches=True):
    """Keys with the screen on, asserted equal (records too) to the screen-off and the plain
    pipeline's; returns them with the screened search's two stats."""
    eng.set_gallery(g, global_offset=offset)
    k_off, m_off, st_off, ss_off = _search(eng, q, 0, 1, matches)
    assert st_off == (len(q), 0, 0, 0) and ss_off == (0, 0, 0)
    k_spl, m_spl, st_spl, ss_spl = _search(eng, q, k1, 0, matches)
    assert ss_spl == (0, 0, 0)
    k_scr, m_scr, st, ss = _search(eng, q, k1, 1, matches)
    for k, m in ((k_spl, m_spl), (k_scr, m_scr)):
        assert np.array_equal(k, k_off)
        if matches:
            assert np.array_equal(m, m_off)
    assert st[0] == len(q) and st[1] + st[2] == len(q) and st[3] == 0
    assert st[2] <= st_spl[2]  # whatever the split stage proves alone, the cascade proves
    assert ss[0] == len(q) and 0 <= ss[1] <= st[1] and ss[2] == 0
    return k_scr, st, ss


def _idx(keys, offset=0):
    return (keys & 0xFFFFFFFF).astype(np.int64) - offset


def _decaying(n, b, k, seed):
    """The data of tests/test_gpu_search_prefix.py: a decaying spectrum, probes planted at
    N(0, 2^2) from a row, every 7th probe unplanted."""
    rng = np.random.default_rng(seed)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    t = rng.integers(0, n, b)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    q[::7] = rng.standard_normal((len(q[::7]), k)).astype(np.float32) * s  # no planted row
    return g, q


# ---- 1. parity grid -----------------------------------------------------------------------
_SHAPES = [(40, 70, 128, 0), (769, 257, 128, 0), (3001, 300, 100, 1000), (3001, 300, 50, 0), (900, 130, 32, 0)]
# K1 16 and 32 where shorter than the padded k (128, 64 at k = 50, 32 at k = 32)
_GRID = [s + (k1,) for s in _SHAPES for k1 in (16, 32) if k1 < (32 if s[2] <= 32 else 64 if s[2] <= 64 else 128)]


@pytest.mark.parametrize("n,b,k,offset,k1", _GRID)
def test_parity_grid(eng, n, b, k, offset, k1):
    g, q = _decaying(n, b, k, n + k)
    keys, st, ss = _three_ways(eng, g, q, k1, offset)
    print(f"stats {st} screen {ss}")
    assert_exact_argbest(q, g, _idx(keys, offset), "l2")


# ---- 2. kernel shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("k1", [16, 32])
def test_three_tiles_per_chunk_and_empty_chunks(eng, k1):
    """4096 probes are 8 probe tiles of 512, so the plan cuts the gallery into 64 chunks
    (search_plan: about 512 workgroups); 130 tiles of 256 rows make chunks of 3 tiles (both LDS
    buffers and the prefetch under way), the last used one of 1 tile of 5 rows, and 20 chunks
    stay empty."""
    n, b, k = 129 * 256 + 5, 4096, 128
    tiles, nchunks = -(-n // 256), 64
    assert -(-tiles // nchunks) == 3 and -(-tiles // 3) < nchunks
    g = synth.gallery_rows(0, n, k)
    rng = np.random.default_rng(n)
    t = rng.integers(0, n, b)
    t[:8] = [0, 255, 256, 767, 768, n - 6, n - 5, n - 1]  # tile edges and the tail tile
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    keys, st, ss = _three_ways(eng, g, q, k1, matches=False)
    print(f"stats {st} screen {ss}")
    np.testing.assert_array_equal(_idx(keys), t)
    assert st[1] >= b - 50  # 16 components do not separate every probe among 33029 rows
    if k1 == 32:
        assert st == (b, b, 0, 0) and ss == (b, b, 0)


@pytest.mark.parametrize("n,b", [(255, 64), (257, 64), (300, 1), (1500, 256), (1500, 700)])
@pytest.mark.parametrize("k1", [16, 32])
def test_edges(eng, n, b, k1):
    """Under one tile; a tail tile of one row; so few tiles that most chunks are empty; one probe;
    256 and 700 probes, where the last workgroup's upper four waves own no probe."""
    g, q = _decaying(n, b, 128, 31 * n + b)
    q[0] = g[n - 1] + 0.5  # the last row wins somewhere
    keys, st, ss = _three_ways(eng, g, q, k1)
    assert_exact_argbest(q, g, _idx(keys), "l2")
    assert _idx(keys)[0] == n - 1


# ---- 3. the bound is the documented one ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bound_batches(n=2048, k=128, k1=32, per=1500, seed=16):
    """Gallery, batch A (0 < margin < es (q1 + g1n(w)) / 4) and batch B (margin above 4 x the
    bound of the pair with the longest row, es (q1 + g1n) + slack), the exact margin
    q1 + min_{g != t} S1(g) - D(t) in NumPy fp64 on the fp32 data."""
    rng = np.random.default_rng(seed)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    g64 = g.astype(np.float64)
    gg1 = (g64[:, :k1] ** 2).sum(1)
    qs, ts = [], []
    for scale in (2.0, 5.0, 6.0, 7.0, 8.0):
        t = rng.integers(0, n, per)
        qs.append((g[t] + scale * rng.standard_normal((per, k))).astype(np.float32))
        ts.append(t)
    q, t = np.concatenate(qs), np.concatenate(ts)
    q64 = q.astype(np.float64)
    rows = np.arange(len(q))
    s1 = gg1[None, :] - 2.0 * q64[:, :k1] @ g64[:, :k1].T
    s1[rows, t] = np.inf
    q1 = (q64[:, :k1] ** 2).sum(1)
    margin = q1 + s1.min(1) - ((q64 - g64[t]) ** 2).sum(1)
    a = np.flatnonzero((margin > 0) & (margin < 0.25 * ps.ES * (q1 + gg1[t])))[:64]
    b = np.flatnonzero(margin > 4.0 * ps.bound(k1, q1, gg1.max()))[:64]
    return g, q[a], t[a], q[b], t[b]


def test_bound_is_the_documented_one(eng):
    """A probe whose exact margin exceeds 4 x the screen's bound must be proven by the screen
    (the proof needs less than twice the bound: the probe's share once, a row's share twice);
    one whose margin is under a quarter of es (q1 + g1n(w)) must not be, and comes back with
    the same key through the later stages."""
    g, qa, ta, qb, tb = _bound_batches()
    print(f"batch A {len(qa)} probes, batch B {len(qb)} probes")
    assert len(qa) >= 16 and len(qb) >= 16
    eng.set_gallery(g)
    for q, t, proven in ((qa, ta, 0), (qb, tb, len(qb))):
        k_off, _, _, _ = _search(eng, q, 0, 1, matches=False)
        k_scr, _, st, ss = _search(eng, q, 32, 1, matches=False)
        print(f"stats {st} screen {ss}")
        assert ss == (len(q), proven, 0)
        assert np.array_equal(k_scr, k_off)
        np.testing.assert_array_equal(_idx(k_scr), t)


def test_outlier_norm_row_costs_the_others_nothing(eng):
    """One row of 1000 x the norm: a bound taken with the gallery's largest norm (es 2 ||q|| gm)
    would be 1000 x wider and prove nothing; the per-row bound still proves the planted probes."""
    n, b, k, k1 = 4096, 256, 128, 32
    g = synth.gallery_rows(0, n, k).copy()
    g[1234] *= np.float32(1000.0)
    rng = np.random.default_rng(1234)
    t = rng.integers(0, n, b)
    t[t == 1234] = 7
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    proven, w, _ = ps.screen_proves(q, g, k1)
    assert proven.all() and np.array_equal(w, t)  # the restated screen proves them all
    keys, st, ss = _three_ways(eng, g, q, k1)
    print(f"stats {st} screen {ss}")
    np.testing.assert_array_equal(_idx(keys), t)
    assert ss == (b, b, 0) and st == (b, b, 0, 0)


# ---- 4. harder inputs ---------------------------------------------------------------------
def test_near_ties_below_the_split_resolution(eng):
    """The data of test_gpu_search_prefix_split's test of that name: twin rows that differ by
    relative 2^-17 .. 2^-20 in prefix components, exact duplicates, and probes equal to such
    rows.  None is proven by the screen (nor by the split stage), keys are the plain pipeline's,
    lowest index first."""
    n, k, k1 = 1024, 128, 32
    rng = np.random.default_rng(1024)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    q, used = [], {33, 777, 801, 44}
    for j, e in enumerate((17, 18, 19, 20) * 4):
        a, b = 10 + 50 * j, 990 - 13 * j
        if j % 2:
            a, b = b, a
        assert not {a, b} & used
        used |= {a, b}
        cols = rng.choice(k1, 1 + j % 5, replace=False)
        g[b] = g[a]
        g[b, cols] = g[a, cols] * np.float32(1.0 + (-1.0) ** j * 2.0 ** -e)
        assert not np.array_equal(g[a], g[b])
        q += [g[a], g[b], g[a] + 0.01 * rng.standard_normal(k).astype(np.float32)]
    for a, b in ((33, 777), (801, 44)):
        g[b] = g[a]
        q += [g[a], g[a] + 0.01 * rng.standard_normal(k).astype(np.float32)]
    q = np.stack(q).astype(np.float32)
    keys, st, ss = _three_ways(eng, g, q, k1)
    assert ss == (len(q), 0, 0) and st == (len(q), 0, len(q), 0)
    assert_exact_argbest(q, g, _idx(keys), "l2")
    assert list(_idx(keys)[-4:]) == [33, 33, 44, 44]


@pytest.mark.parametrize("case", ["nan", "inf", "2^40", "2^-40"])
def test_irregular_and_scaled_galleries(eng, case):
    g, q = _decaying(3000, 200, 128, 40)
    if case == "nan":
        g[17, 3] = np.nan
    elif case == "inf":
        g[2999, 100] = np.inf
        g[5, 0] = -np.inf
    else:
        f = np.float32(2.0 ** (40 if case == "2^40" else -40))
        g, q = g * f, q * f
    keys, st, ss = _three_ways(eng, g, q, 32)
    print(f"stats {st} screen {ss}")
    if case in ("nan", "inf"):
        assert ss == (len(q), 0, 0)  # outside the bound's domain nothing is proven from scores
    else:
        assert ss[1] > 100
        assert_exact_argbest(q, g, _idx(keys), "l2")


# ---- 5. planted data, guard, option -------------------------------------------------------
def test_planted_decaying_spectrum_all_proven_by_the_screen(eng):
    """65536 rows, 512 probes, K1 = 32 (tests/test_prefix_screen_cpu.py proves all 512 with the
    restated screen): the screen proves every probe, nothing is left for the later stages."""
    n, k, b, k1 = 65536, 128, 512, 32
    g = synth.gallery_rows(0, n, k)
    rng = np.random.default_rng(512)
    t = rng.integers(0, n, b)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    eng.set_gallery(g)
    k_off, _, _, _ = _search(eng, q, 0, 1, matches=False)
    k_scr, _, st, ss = _search(eng, q, k1, 1, matches=False)
    assert ss == (b, b, 0) and st == (b, b, 0, 0)
    assert np.array_equal(k_scr, k_off)
    np.testing.assert_array_equal(_idx(k_scr), t)


@functools.lru_cache(maxsize=None)
def _guard_data(n=4096, b=512, k=128, k1=32, twins=300):
    """A gallery and probes that the split stage proves and the screen cannot: the `twins` rows
    of largest prefix norm each get a twin at squared distance 9.5^2 = 90.25 (one prefix column),
    written over the rows of smallest norm, and are their own probes.  The exact margin is 90.25:
    above the split bound (delta1 <= 56 on this spectrum) and under the screen's es (q1 + g1n) >=
    180 for rows of g1n >= 11500.  The other probes are planted at N(0, 2^2) as everywhere."""
    g = synth.gallery_rows(0, n, k).copy()
    g1 = (g[:, :k1].astype(np.float64) ** 2).sum(1)
    order = np.argsort(g1)
    a, tw = order[-twins:], order[:twins]
    assert g1[a].min() >= 11500.0
    g[tw] = g[a]
    g[tw, 20] += np.float32(9.5)
    rng = np.random.default_rng(99)
    t = rng.choice(order[twins:-twins], b - twins, replace=False)
    q = np.concatenate([g[a], (g[t] + 2.0 * rng.standard_normal((b - twins, k))).astype(np.float32)])
    want = np.concatenate([np.minimum(a, a), t])
    perm = rng.permutation(b)
    return g, q[perm], want[perm]


def test_screen_guard(eng):
    """A search in which the screen leaves more than half of the probes (300 of 512) to the split
    stage, which proves them: the next search goes straight to the split stage, with the same
    keys; setting the option clears the guard."""
    g, q, want = _guard_data()
    b = len(q)
    eng.set_gallery(g)
    k_off, _, _, _ = _search(eng, q, 0, 1, matches=False)
    np.testing.assert_array_equal(_idx(k_off), want)
    k1, _, st1, ss1 = _search(eng, q, 32, 1, matches=False)
    print(f"stats {st1} screen {ss1}")
    assert ss1[0] == b and 2 * ss1[1] < b and ss1[2] == 0
    assert st1[1] >= b - 20 and st1[3] == 0  # the split stage proves them; the prefix guard stays quiet
    k2 = eng.search_keys(q)  # search_stats above synchronised: the counters have arrived
    st2, ss2 = eng.search_stats(), eng.search_screen_stats()
    assert ss2 == (0, 0, 1) and st2 == st1
    assert np.array_equal(k1, k_off) and np.array_equal(k2, k_off)
    eng.set_option("search_prefix_screen", 1)
    k3 = eng.search_keys(q)
    assert eng.search_screen_stats() == ss1 and np.array_equal(k3, k_off)


def test_option_roundtrip_and_range(eng):
    assert eng.get_option("search_prefix_screen") == 1
    for v in (0, 1):
        eng.set_option("search_prefix_screen", v)
        assert eng.get_option("search_prefix_screen") == v
    for v in (2, -1, 16):
        with pytest.raises(EigenfaceError) as err:
            eng.set_option("search_prefix_screen", v)
        assert err.value.code == EF_E_INVALID
    assert eng.get_option("search_prefix_screen") == 1
    assert eng.get_option("search_prefix_split") == 1
