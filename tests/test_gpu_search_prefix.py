"""Prefix scan (EF_OPT_SEARCH_PREFIX): L2 matches are decided from the first K1 components
of every row where that proves them, and by the full-k pipeline where it does not.  Keys and
match records must equal option 0's bit for bit on every input, and the fp64 arg-min with
lowest-index ties (tests/parity_util.py, NumPy)."""
import functools

import numpy as np
import pytest

from eigenface import synth
from eigenface._native import EigenfaceError
from parity_util import assert_exact_argbest, top2

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_option(eng):
    yield
    eng.set_option("search_prefix", 1)


def _on_vs_off(eng, g, q, k1, metric="l2", offset=0):
    """Keys with the prefix scan at K1 (asserted equal to option 0's, records too) and the
    stats of the keys search.  Setting the option clears the guard, so every search with the
    option on really runs the prefix scan."""
    eng.set_option("search_prefix", 0)
    eng.set_gallery(g, global_offset=offset)
    k_off = eng.search_keys(q, metric)
    m_off = eng.search_matches(q, metric)
    assert eng.search_stats() == (len(q), 0, 0, 0)
    eng.set_option("search_prefix", k1)
    k_on = eng.search_keys(q, metric)
    st = eng.search_stats()
    eng.set_option("search_prefix", k1)
    m_on = eng.search_matches(q, metric)
    assert np.array_equal(k_on, k_off)
    assert np.array_equal(m_on, m_off)
    assert st[0] == len(q) and st[3] == 0
    if metric == "l2":
        assert st[1] + st[2] == len(q)
    else:
        assert st[1] == st[2] == 0
    return k_on, st


def _idx(keys, offset=0):
    return (keys & 0xFFFFFFFF).astype(np.int64) - offset


def _argmin64(q, g):
    """NumPy fp64 squared distances in difference form, first index among exact ties."""
    g64 = g.astype(np.float64)
    return np.array([np.argmin(((x.astype(np.float64) - g64) ** 2).sum(1)) for x in q])


@functools.lru_cache(maxsize=None)
def _flat(k):
    rng = np.random.default_rng(20037 + k)
    g = rng.standard_normal((20037, k)).astype(np.float32)
    q = rng.standard_normal((300, k)).astype(np.float32)
    for a in (g, q):
        a.setflags(write=False)
    return g, q, top2(q, g, "l2")


@pytest.mark.parametrize("k1", [16, 32, 64])
@pytest.mark.parametrize("k", [128, 100])
def test_flat_spectrum_random_probes(eng, k, k1):
    """Nothing separates in the prefix, so nearly every probe takes the full-k run: a ragged
    probe tile (300), the tail gallery tile (20037 = 313 x 64 + 5) and several chunks."""
    g, q, ref = _flat(k)
    keys, st = _on_vs_off(eng, g, q, k1)
    assert_exact_argbest(q, g, _idx(keys), "l2", ref=ref)
    assert st[2] > 150  # the second run is what this case is about


def test_planted_decaying_spectrum(eng):
    """The benchmark's spectrum at one generator block: probes are gallery rows plus N(0, 2^2)
    per feature.  Every probe whose smallest non-target prefix distance exceeds 1.01 x its
    target's full distance (NumPy fp64) must be proven by the prefix scan."""
    n, k, b, k1 = 65536, 128, 512, 32
    g = synth.gallery_rows(0, n, k)
    rng = np.random.default_rng(512)
    t = rng.integers(0, n, b)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    keys, st = _on_vs_off(eng, g, q, k1)
    np.testing.assert_array_equal(_idx(keys), t)
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    d_t = ((q64 - g64[t]) ** 2).sum(1)
    qq1 = (q64[:, :k1] ** 2).sum(1)
    rival = np.full(b, np.inf)
    for a in range(0, n, 8192):
        gc = g64[a:a + 8192, :k1]
        d1 = qq1[:, None] + (gc ** 2).sum(1)[None, :] - 2.0 * q64[:, :k1] @ gc.T
        own = (t >= a) & (t < a + len(gc))
        d1[np.flatnonzero(own), t[own] - a] = np.inf
        rival = np.minimum(rival, d1.min(1))
    provable = int((rival > 1.01 * d_t).sum())
    print(f"provable {provable} of {b}, stats {st}, smallest ratio {np.min(rival / d_t):.3f}")
    assert provable > 0
    assert st[1] >= provable


@pytest.mark.parametrize("k1", [16, 32, 64])
def test_constructed_rows(eng, k1):
    n, k = 4096, 128
    rng = np.random.default_rng(4096 + k1)
    g = rng.standard_normal((n, k)).astype(np.float32)
    tail = lambda s=1.0: (s * rng.standard_normal(k - k1)).astype(np.float32)  # noqa: E731
    q = rng.standard_normal((40, k)).astype(np.float32)
    want = {}
    # (a) rows 100 < 2000 equal in the prefix, differing after; the probe is nearer row 2000
    g[2000, :k1] = g[100, :k1]
    q[0] = g[2000]
    q[0, k1:] += 0.01 * tail()
    want[0] = 2000
    # (b) row 300 matches the probe's prefix exactly but is far in the tail; row 3000 is a
    # little off everywhere and the true nearest
    q[1] = g[3000] + 0.05 * rng.standard_normal(k).astype(np.float32)
    g[300, :k1] = q[1, :k1]
    g[300, k1:] = q[1, k1:] + tail(3.0)
    want[1] = 3000
    # (c) exact duplicate rows: the lowest index wins
    g[[700, 1500, 3900]] = g[700]
    q[2] = g[700] + 0.01 * rng.standard_normal(k).astype(np.float32)
    q[3] = g[700]
    want[2] = want[3] = 700
    # (d) 100 rows sharing a prefix with distinct tails (more than the candidate list holds)
    rows = np.arange(1000, 1100)
    g[rows, :k1] = g[1000, :k1]
    for r in rows:
        g[r, k1:] = g[1000, k1:] + tail(0.1)
    q[4] = g[1057]
    q[4, k1:] += 0.001 * tail()
    q[5] = g[1099]
    want[4], want[5] = 1057, 1099
    keys, st = _on_vs_off(eng, g, q, k1)
    idx = _idx(keys)
    np.testing.assert_array_equal(idx, _argmin64(q, g))
    for p, r in want.items():
        assert idx[p] == r, (p, idx[p], r)
    assert st[2] >= 5  # (a), (c) and (d) tie in the prefix and cannot be proven by it


def _decaying(n, b, k, seed):
    rng = np.random.default_rng(seed)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    t = rng.integers(0, n, b)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    q[::7] = rng.standard_normal((len(q[::7]), k)).astype(np.float32) * s  # no planted row
    return g, q


@pytest.mark.parametrize("n,b,k,offset", [(40, 70, 128, 0), (769, 257, 128, 0), (3001, 300, 100, 1000),
                                          (3001, 300, 50, 0)])
def test_sizes_and_offsets(eng, n, b, k, offset):
    """Under one tile; 769 rows x 257 probes (13 tiles in 16 chunks, three of them empty);
    a gallery with a global offset; padded k = 64."""
    g, q = _decaying(n, b, k, n + k)
    keys, st = _on_vs_off(eng, g, q, 32, offset=offset)
    assert_exact_argbest(q, g, _idx(keys, offset), "l2")
    assert st[1] > 0 and st[2] > 0  # both ways out of the proof are taken


def test_gallery_replaced(eng):
    """The prefix copy follows the gallery: a second gallery of the same shape."""
    ga, q = _decaying(5000, 300, 128, 1)
    gb, _ = _decaying(5000, 300, 128, 2)
    eng.set_option("search_prefix", 32)
    eng.set_gallery(ga)
    ka = eng.search_keys(q)
    assert eng.search_stats()[1] > 200  # the probes are planted in the first gallery
    eng.set_gallery(gb)
    kb = eng.search_keys(q)
    eng.set_option("search_prefix", 0)
    np.testing.assert_array_equal(kb, eng.search_keys(q))
    eng.set_gallery(ga)
    np.testing.assert_array_equal(ka, eng.search_keys(q))
    assert_exact_argbest(q, gb, _idx(kb), "l2")
    assert not np.array_equal(ka, kb)


def test_option_roundtrip_and_range(eng):
    g, _ = _decaying(100, 1, 128, 3)
    eng.set_gallery(g)
    assert eng.get_option("search_prefix") == 1
    for v in (0, 16, 32, 64, 1):
        eng.set_option("search_prefix", v)
        assert eng.get_option("search_prefix") == v
    for v in (48, 128, -1, 2):
        with pytest.raises(EigenfaceError):
            eng.set_option("search_prefix", v)
    assert eng.get_option("search_prefix") == 1


def test_cosine_unaffected(eng):
    g, q = _decaying(3001, 300, 128, 4)
    keys, st = _on_vs_off(eng, g, q, 32, metric="cosine")
    assert_exact_argbest(q, g, _idx(keys), "cosine")


def test_guard_skips_after_a_fallback_heavy_search(eng):
    g, q, _ = _flat(128)
    eng.set_option("search_prefix", 0)
    eng.set_gallery(g)
    k_off = eng.search_keys(q)
    eng.set_option("search_prefix", 32)
    k_first = eng.search_keys(q)
    first = eng.search_stats()
    assert first[3] == 0 and 2 * -(-first[2] // 256) > -(-len(q) // 256)
    k_next = eng.search_keys(q)  # the first search's counters are on the host by now
    assert eng.search_stats() == (len(q), 0, 0, 1)
    np.testing.assert_array_equal(k_first, k_off)
    np.testing.assert_array_equal(k_next, k_off)
