"""Split-bf16 prefix scan (EF_OPT_SEARCH_PREFIX_SPLIT, the default): the prefix scan of
EF_OPT_SEARCH_PREFIX on bf16 matrix cores with split (hi + lo) operands and the split chain's
bound.  Keys and match records must equal the fp32 prefix scan's (option 0) and the plain
full-k pipeline's bit for bit, and the proof must use the documented bound."""
import functools

import numpy as np
import pytest

from eigenface import synth
from eigenface._native import EigenfaceError
from parity_util import assert_exact_argbest, top2

pytestmark = pytest.mark.gpu
EF_E_INVALID = -1  # include/eigenface.h


@pytest.fixture(autouse=True)
def _default_options(eng):
    yield
    eng.set_option("search_prefix", 1)
    eng.set_option("search_prefix_split", 1)


def _search(eng, q, k1, split, matches=True):
    """(keys, records, stats of the keys search) at prefix length k1 (0: no prefix scan) in
    the given arithmetic.  Setting the option clears the guard before each search."""
    eng.set_option("search_prefix_split", split)
    eng.set_option("search_prefix", k1)
    keys = eng.search_keys(q)
    st = eng.search_stats()
    m = None
    if matches:
        eng.set_option("search_prefix", k1)
        m = eng.search_matches(q)
    return keys, m, st


def _three_ways(eng, g, q, k1, offset=0):
    """Keys under the split prefix scan, asserted equal (records too) to the fp32 prefix
    scan's and to the plain pipeline's; returns them with the split search's stats."""
    eng.set_gallery(g, global_offset=offset)
    k_off, m_off, st_off = _search(eng, q, 0, 1)
    assert st_off == (len(q), 0, 0, 0)
    k_f32, m_f32, st_f32 = _search(eng, q, k1, 0)
    k_spl, m_spl, st_spl = _search(eng, q, k1, 1)
    for k, m, st in ((k_f32, m_f32, st_f32), (k_spl, m_spl, st_spl)):
        assert np.array_equal(k, k_off)
        assert np.array_equal(m, m_off)
        assert st[0] == len(q) and st[1] + st[2] == len(q) and st[3] == 0
    return k_spl, st_spl


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
_SHAPES = [(40, 70, 128, 0), (769, 257, 128, 0), (3001, 300, 100, 1000), (3001, 300, 50, 0)]


# every K1 shorter than the padded k (64 at k = 50, else 128)
_GRID = [s + (k1,) for s in _SHAPES for k1 in (16, 32, 64) if k1 < (64 if s[2] <= 64 else 128)]


@pytest.mark.parametrize("n,b,k,offset,k1", _GRID)
def test_parity_grid(eng, n, b, k, offset, k1):
    """Under one tile; a ragged probe tile with the tail gallery tile and empty chunks; a
    global offset; padded k = 64."""
    g, q = _decaying(n, b, k, n + k)
    keys, st = _three_ways(eng, g, q, k1, offset)
    assert_exact_argbest(q, g, _idx(keys, offset), "l2")


@functools.lru_cache(maxsize=None)
def _flat():
    rng = np.random.default_rng(20037 + 128)
    g = rng.standard_normal((20037, 128)).astype(np.float32)
    q = rng.standard_normal((300, 128)).astype(np.float32)
    return g, q, top2(q, g, "l2")


@pytest.mark.parametrize("k1", [16, 32, 64])
def test_flat_spectrum(eng, k1):
    """Nothing separates in the prefix: most probes take the second run."""
    g, q, ref = _flat()
    keys, st = _three_ways(eng, g, q, k1)
    assert_exact_argbest(q, g, _idx(keys), "l2", ref=ref)
    assert st[2] > 150


# ---- 2. the bound is the documented one ---------------------------------------------------
def _split_delta(k1, qn, gmax2, b1):
    """2 x scan_delta<L2, split> of DESIGN.md K8p, in fp64: e1 = the split chain's bound
    (dropped terms, 3 K1 + 4 adds at 2u, the fp32 norm, the final rounding), scan_delta =
    4 e1, and the proof's delta1 doubles it."""
    u = 2.0 ** -24
    es = 3.05 * 2.0 ** -16
    gm = np.sqrt(gmax2)
    e1 = 2 * es * qn * gm + (3 * k1 + 4) * 2 * u * 1.01 * (2.02 * qn * gm + gmax2) + k1 * u * gmax2 + 4 * u * np.abs(b1)
    return 2.0 * (4.0 * e1)


@functools.lru_cache(maxsize=None)
def _bound_batches(n=2048, k=128, k1=32, per=4000, seed=7):
    """Gallery, batch A (0 < margin < delta / 4) and batch B (margin > 4 delta), the exact
    margin q1 + min_{g != t} S1(g) - D(t) in NumPy fp64 on the fp32 data."""
    rng = np.random.default_rng(seed)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    g64 = g.astype(np.float64)
    gg1 = (g64[:, :k1] ** 2).sum(1)
    gmax2 = (g64 ** 2).sum(1).max()
    qs, ts = [], []
    for scale in (2.0, 4.5, 5.0, 5.5, 6.0):
        t = rng.integers(0, n, per)
        qs.append((g[t] + scale * rng.standard_normal((per, k))).astype(np.float32))
        ts.append(t)
    q, t = np.concatenate(qs), np.concatenate(ts)
    q64 = q.astype(np.float64)
    rows = np.arange(len(q))
    s1 = gg1[None, :] - 2.0 * q64[:, :k1] @ g64[:, :k1].T
    b1 = s1[rows, t].copy()
    s1[rows, t] = np.inf
    margin = (q64[:, :k1] ** 2).sum(1) + s1.min(1) - ((q64 - g64[t]) ** 2).sum(1)
    delta = _split_delta(k1, np.sqrt((q64 ** 2).sum(1)), gmax2, b1)
    a = np.flatnonzero((margin > 0) & (margin < 0.25 * delta))
    b = np.flatnonzero(margin > 4.0 * delta)[:64]
    return g, q[a], t[a], q[b], t[b]


def test_bound_is_the_documented_one(eng):
    """A probe whose exact margin is under a quarter of delta1 = 2 scan_delta must go to the
    full-k run (the scan's own error is at most delta1 / 8), one whose margin exceeds
    4 delta1 must be proven: the bound is neither tighter nor much wider than documented."""
    g, qa, ta, qb, tb = _bound_batches()
    print(f"batch A {len(qa)} probes, batch B {len(qb)} probes")
    assert len(qa) >= 16 and len(qb) >= 16
    eng.set_gallery(g)
    for q, t, proven in ((qa, ta, 0), (qb, tb, len(qb))):
        k_off, _, _ = _search(eng, q, 0, 1, matches=False)
        k_spl, _, st = _search(eng, q, 32, 1, matches=False)
        print(f"stats {st}")
        assert st == (len(q), proven, len(q) - proven, 0)
        assert np.array_equal(k_spl, k_off)
        np.testing.assert_array_equal(_idx(k_spl), t)


# ---- 3. near-ties below the split's resolution --------------------------------------------
def test_near_ties_below_the_split_resolution(eng):
    """Twin rows that differ only by relative 2^-17 .. 2^-20 in prefix components, exact
    duplicates, and probes equal to such rows: the split scan cannot tell the twins apart,
    so none is proven by the prefix and the answer is the fp64 arg-min, lowest index first."""
    n, k, k1 = 1024, 128, 32
    rng = np.random.default_rng(1024)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    q, used = [], {33, 777, 801, 44}
    for j, e in enumerate((17, 18, 19, 20) * 4):
        a, b = 10 + 50 * j, 990 - 13 * j  # the twin may precede or follow in the scan
        if j % 2:
            a, b = b, a
        assert not {a, b} & used  # no pair overwrites another
        used |= {a, b}
        cols = rng.choice(k1, 1 + j % 5, replace=False)
        g[b] = g[a]
        g[b, cols] = g[a, cols] * np.float32(1.0 + (-1.0) ** j * 2.0 ** -e)
        assert not np.array_equal(g[a], g[b])
        q += [g[a], g[b], g[a] + 0.01 * rng.standard_normal(k).astype(np.float32)]
    for a, b in ((33, 777), (801, 44)):  # exact duplicates: the lower index wins
        g[b] = g[a]
        q += [g[a], g[a] + 0.01 * rng.standard_normal(k).astype(np.float32)]
    q = np.stack(q).astype(np.float32)
    eng.set_gallery(g)
    k_off, m_off, _ = _search(eng, q, 0, 1)
    k_spl, m_spl, st = _search(eng, q, k1, 1)
    assert st == (len(q), 0, len(q), 0)
    assert np.array_equal(k_spl, k_off) and np.array_equal(m_spl, m_off)
    assert_exact_argbest(q, g, _idx(k_spl), "l2")
    assert list(_idx(k_spl)[-4:]) == [33, 33, 44, 44]


# ---- 4. option behaviour ------------------------------------------------------------------
def test_option_roundtrip_and_range(eng):
    assert eng.get_option("search_prefix_split") == 1
    for v in (0, 1):
        eng.set_option("search_prefix_split", v)
        assert eng.get_option("search_prefix_split") == v
    for v in (2, -1, 13):
        with pytest.raises(EigenfaceError) as err:
            eng.set_option("search_prefix_split", v)
        assert err.value.code == EF_E_INVALID
    assert eng.get_option("search_prefix_split") == 1


def test_switching_on_a_live_gallery(eng):
    g, q = _decaying(5000, 300, 128, 1)
    eng.set_gallery(g)
    runs = [_search(eng, q, 32, v, matches=False) for v in (1, 0, 1)]
    for keys, _, st in runs:
        assert np.array_equal(keys, runs[0][0])
        assert st[1] > 200 and st[1] + st[2] == len(q)
    assert_exact_argbest(q, g, _idx(runs[0][0]), "l2")


def test_gallery_replaced(eng):
    """The split copy follows the gallery: a second gallery of the same shape."""
    ga, q = _decaying(5000, 300, 128, 1)
    gb, _ = _decaying(5000, 300, 128, 2)
    eng.set_gallery(ga)
    ka, _, st = _search(eng, q, 32, 1, matches=False)
    assert st[1] > 200  # the probes are planted in the first gallery
    eng.set_gallery(gb)
    kb, _, _ = _search(eng, q, 32, 1, matches=False)
    k_off, _, _ = _search(eng, q, 0, 1, matches=False)
    assert np.array_equal(kb, k_off)
    assert_exact_argbest(q, gb, _idx(kb), "l2")
    assert not np.array_equal(ka, kb)


# ---- 5. the benchmark's spectrum at one generator block -----------------------------------
def test_planted_decaying_spectrum_all_proven(eng):
    """The data of test_planted_decaying_spectrum (65536 rows, 512 probes, K1 = 32).  NumPy
    fp64: the smallest margin is 752.7, the largest scan_delta 28.0 and so the largest
    delta1 = 2 scan_delta 56.0: the split prefix proves all 512."""
    n, k, b, k1 = 65536, 128, 512, 32
    g = synth.gallery_rows(0, n, k)
    rng = np.random.default_rng(512)
    t = rng.integers(0, n, b)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    eng.set_gallery(g)
    k_off, _, _ = _search(eng, q, 0, 1, matches=False)
    k_spl, _, st = _search(eng, q, k1, 1, matches=False)
    assert st == (b, b, 0, 0)
    assert np.array_equal(k_spl, k_off)
    np.testing.assert_array_equal(_idx(k_spl), t)
