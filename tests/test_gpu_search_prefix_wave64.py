"""The split-bf16 prefix scan at K1 <= 32 (prefix64_kernel): 64 probes per wave
in two 32-probe blocks, 512 probes per workgroup, 256-row tiles in swizzled LDS rows, the
probes read from the padded feature rows in place.  Keys and match records must equal the
plain pipeline's (search_prefix 0) and the fp32 prefix scan's (search_prefix_split 0) bit for
bit at every probe count around the 512-probe tile, every row count around tiles and chunks
and every (padded k, K1) pair; planted and tied rows cover every probe slot and row position."""
import functools

import numpy as np
import pytest

from eigenface import synth
from parity_util import assert_exact_argbest
from test_gpu_search_prefix_split import _decaying, _idx, _search, _split_delta, _three_ways

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_options(eng):
    yield
    eng.set_option("search_prefix", 1)
    eng.set_option("search_prefix_split", 1)


@functools.lru_cache(maxsize=None)
def _data(n, b, k):
    g, q = _decaying(n, b, k, 7 * n + k)
    for a in (g, q):
        a.setflags(write=False)
    return g, q


# ---- 1. probe counts around the 512-probe tile ----------------------------------------------
@pytest.mark.parametrize("k1", [16, 32])
@pytest.mark.parametrize("b", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769])
def test_probe_counts(eng, b, k1):
    """One wave, one probe block, both; one, two and three 256-probe pads: 257 and 769 leave a
    last workgroup whose upper four waves own no probe."""
    g, q = _data(1000, 769, 128)
    q = q[:b]
    keys, st = _three_ways(eng, g, q, k1, offset=5000)
    assert_exact_argbest(q, g, _idx(keys, 5000), "l2")


# ---- 2. row counts around tiles and chunks ---------------------------------------------------
@pytest.mark.parametrize("k1", [16, 32])
@pytest.mark.parametrize("n", [1, 31, 33, 255, 256, 257, 511, 513, 2049])
def test_row_counts(eng, n, k1):
    """Under 8 x 256 rows some of the 8 chunks are empty; 257 and 513 end a tail tile inside its
    first row block, 2049 gives every chunk a tile and a ninth, one-row tile."""
    g, q = _data(n, 300, 128)
    keys, st = _three_ways(eng, g, q, k1)
    assert_exact_argbest(q, g, _idx(keys), "l2")


# ---- 3. every (padded k, K1) pair the kernel is built for -------------------------------------
@pytest.mark.parametrize("k,k1", [(128, 32), (128, 16), (64, 32), (64, 16), (32, 16)])
def test_every_kp_k1_pair(eng, k, k1):
    g, q = _data(777, 130, k)
    keys, st = _three_ways(eng, g, q, k1)
    assert_exact_argbest(q, g, _idx(keys), "l2")


# ---- 4. every probe slot and every row position ----------------------------------------------
@pytest.mark.parametrize("k1", [16, 32])
def test_every_probe_slot_and_row_position(eng, k1):
    """512 probes, each planted on a row of its own: probes p and p + 256 win at tile position
    p % 256 of different tiles, so the winners cover all 256 positions of a tile (every row
    block, both lane halves, every accumulator register) from both probe blocks of every wave.
    The benchmark's decaying spectrum with N(0, 2^2) noise: every probe is proven."""
    n, k, b = 2048 + 100, 128, 512
    g = synth.gallery_rows(0, n, k)
    p = np.arange(b)
    t = (p % 256) + 256 * ((p % 8 + p // 256) % 8)
    assert len(set(t)) == b and set(t % 256) == set(range(256))
    rng = np.random.default_rng(2148)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    keys, st = _three_ways(eng, g, q, k1, offset=77)
    print(f"stats {st}")
    np.testing.assert_array_equal(_idx(keys, 77), t)
    assert st == (b, b, 0, 0)


# ---- 5. the tie rule --------------------------------------------------------------------------
def test_exact_duplicates_name_the_lowest_index(eng):
    """Exact duplicate rows in the two lane halves of one 32-row block, in the two blocks a wave
    runs at once, in different block pairs of a tile, in consecutive tiles and in tiles far
    apart.  A duplicate is the runner-up at the winner's own score, so the prefix proves none
    of these probes and the key names the lower index.  Alone the 14 probes make one probe
    tile, which gets every 256-row tile as a chunk of its own; among 64 probe tiles the 16
    tiles make 8 chunks of 2 (search_plan), so the pairs in tiles (0, 1) and (4, 5) meet in one
    workgroup's sweep, through both LDS buffers, and the others in different chunks."""
    n, k = 4096, 128
    rng = np.random.default_rng(4096)
    s = synth.spectrum(k).astype(np.float32)
    g = rng.standard_normal((n, k)).astype(np.float32) * s
    pairs = [(3, 7), (9, 41), (1024, 1152), (100, 400), (1279, 1280), (450, 3000), (600, 4095)]
    assert len({r for p in pairs for r in p}) == 2 * len(pairs)
    q = []
    for a, b in pairs:
        assert a < b
        g[b] = g[a]
        q += [g[a], g[a] + 0.01 * rng.standard_normal(k).astype(np.float32)]
    q = np.stack(q).astype(np.float32)
    want = [a for a, _ in pairs for _ in range(2)]
    # planted probes around them: 64 tiles of 512, the duplicates' probes spread over the batch
    b = 64 * 512
    t = rng.integers(0, n, b)
    big = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    at = np.arange(len(q)) * 2339 + 31
    big[at] = q
    for k1 in (16, 32):
        keys, st = _three_ways(eng, g, q, k1)
        assert st == (len(q), 0, len(q), 0)
        assert list(_idx(keys)) == want
        keys, st = _three_ways(eng, g, big, k1)
        assert st[2] >= len(q)
        assert list(_idx(keys)[at]) == want
    assert_exact_argbest(q, g, _idx(keys)[at], "l2")


# ---- 6. the proof's two sides at the new shapes -----------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_sided_batch(n=2048, k=128, k1=32, per=4000, seed=11, b=513):
    """A gallery and b probes, each with an exact margin (NumPy fp64 on the fp32 data, as
    test_bound_is_the_documented_one forms it) either in (0, delta1 / 4) or above 4 delta1,
    delta1 = 2 scan_delta<L2, split>: at least 16 of the first kind, spread over the batch."""
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
    low = np.flatnonzero((margin > 0) & (margin < 0.25 * delta))[:128]
    high = np.flatnonzero(margin > 4.0 * delta)[: b - len(low)]
    assert len(low) >= 16 and len(low) + len(high) == b
    pick = np.concatenate([low, high])
    pick = pick[np.random.default_rng(b).permutation(b)]  # both kinds in every wave and probe block
    return g, q[pick], t[pick], np.isin(pick, high)


def test_bound_both_sides_with_a_half_dead_workgroup(eng):
    """513 probes = one full 512-probe workgroup and one with a single probe block in use and
    four waves without probes.  Probes whose exact margin exceeds 4 delta1 must be proven,
    those under delta1 / 4 must go to the full-k run — the documented bound, unchanged."""
    g, q, t, proven = _two_sided_batch()
    n_proven = int(proven.sum())
    print(f"{len(q)} probes, {n_proven} to be proven, {len(q) - n_proven} to be listed")
    keys, st = _three_ways(eng, g, q, 32)
    print(f"stats {st}")
    np.testing.assert_array_equal(_idx(keys), t)
    assert st == (len(q), n_proven, len(q) - n_proven, 0)
    # each side alone: all proven, none proven
    for sel, want in ((proven, n_proven), (~proven, 0)):
        eng.set_gallery(g)
        k_one, _, st_one = _search(eng, q[sel], 32, 1, matches=False)
        assert st_one == (int(sel.sum()), want, int(sel.sum()) - want, 0)
        assert np.array_equal(k_one, keys[sel])
