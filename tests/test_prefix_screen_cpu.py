"""The single-bf16 prefix screen without a GPU: its score and its per-row bound restated in NumPy
and torch bf16 (prefix_screen_util), the planted benchmark data, and the symbols."""
import ctypes
import os
import re

import numpy as np
import pytest

import prefix_screen_util as ps
from eigenface import _native as N
from eigenface import synth

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _rows(kind, n, k, rng):
    g = rng.standard_normal((n, k))
    if kind == "decaying":
        g *= synth.spectrum(k)
    elif kind == "outlier":
        g *= synth.spectrum(k)
        g[n // 3] *= 1000.0  # one row of 1000 x the norm
    return g


@pytest.mark.parametrize("k1", (16, 32))
@pytest.mark.parametrize("kind", ("decaying", "flat", "outlier"))
@pytest.mark.parametrize("scale", (2.0 ** -30, 1.0, 2.0 ** 30))
def test_bound_holds_for_every_pair(scale, kind, k1):
    """|S~1 - S1| <= es (q1 + g1n) + slack for every (probe, row) pair, S~1 the fp32 chain of
    bf16 products from the fp32 norm and S1 in fp64; and the chain from the start value is a
    lower bound: L <= S1 + (es + cq) q1."""
    n, b, k = 192, 48, 64
    rng = np.random.default_rng(k1 + len(kind))
    g = (_rows(kind, n, k, rng) * scale).astype(np.float32)
    t = rng.integers(0, n, b)
    q = g[t] + (2.0 * scale) * rng.standard_normal((b, k))
    q[::5] = _rows(kind, len(q[::5]), k, rng) * scale  # unplanted probes too
    q[1] = g[n // 3]  # the long row itself (outlier) as a probe
    q = q.astype(np.float32)
    s1 = ps.exact_s1(q, g, k1)
    q1 = (q[:, :k1].astype(np.float64) ** 2).sum(1)[:, None]
    g1 = (g[:, :k1].astype(np.float64) ** 2).sum(1)[None, :]
    gn1 = ps.norms1(g, k1)
    err = np.abs(ps.chain(gn1, q, g, k1).astype(np.float64) - s1)
    bnd = ps.bound(k1, q1, g1)
    assert (err <= bnd).all(), float((err / bnd).max())
    assert (err / bnd).max() > 1e-3  # the rounding was exercised
    L = ps.chain(ps.start_values(gn1, k1), q, g, k1).astype(np.float64)
    assert (L <= s1 + (ps.ES + ps.cq(k1)) * q1).all()
    # the lower bound is not vacuous: within 2 (es + cg) g1n + 2 (es + cq) q1 of the score
    assert (L >= s1 - 2.0 * bnd).all()


def test_planted_benchmark_data_all_proven():
    """The data of test_planted_decaying_spectrum_all_proven (65536 rows, 512 probes, K1 = 32):
    the screen's test proves 512 of 512, each with the planted row."""
    n, k, b, k1 = 65536, 128, 512, 32
    g = synth.gallery_rows(0, n, k)
    rng = np.random.default_rng(512)
    t = rng.integers(0, n, b)
    q = (g[t] + 2.0 * rng.standard_normal((b, k))).astype(np.float32)
    proven, w, margin = ps.screen_proves(q, g, k1)
    print(f"proven {int(proven.sum())} of {b}, smallest margin {margin.min():.1f}")
    assert proven.all()
    np.testing.assert_array_equal(w, t)


def test_symbols():
    with open(os.path.join(ROOT, "include", "eigenface.h")) as f:
        hdr = f.read()
    assert "#define EF_API_VERSION 7" in hdr
    assert re.search(r"#define EF_OPT_SEARCH_PREFIX_SCREEN 16\b", hdr) and N.EF_OPT_SEARCH_PREFIX_SCREEN == 16
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    assert "int ef_prefix_screen_stats(ef_ctx* ctx, int64_t out[3]);" in flat
    assert N._SIGS["ef_prefix_screen_stats"] == ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)], ctypes.c_int)
    assert hasattr(N.lib(), "ef_prefix_screen_stats")
    from eigenface import engine
    assert engine._OPTIONS["search_prefix_screen"] == 16
    assert hasattr(engine.Engine, "search_screen_stats")
