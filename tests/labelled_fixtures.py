"""Inputs of the labelled-search tests (tests/test_gpu_search_labelled.py), generated once per
shape and shared, each with its fp64 reference (labelled_util)."""
import functools

import numpy as np

import labelled_util as lu
import parity_util as pu

B = 300
RELATIONS = ("same", "other", "any")
METRICS = ("l2", "cosine")


@functools.lru_cache(maxsize=None)
def random_case(k, n):
    """Test 1's data: gallery, probes, labels 0..6 on rows and 0..7 on probes (7 is in no
    gallery), exclusions in -1..n-1 (-1 excludes nothing)."""
    rng = np.random.default_rng(1000 * k + n)
    g = rng.standard_normal((n, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    glab = rng.integers(0, 7, n).astype(np.int32)
    plab = rng.integers(0, 8, B).astype(np.int32)
    excl = rng.integers(-1, n, B).astype(np.int64)
    return g, q, glab, plab, excl


@functools.lru_cache(maxsize=None)
def random_refs(k, n, metric):
    """{relation: fp64 reference} of random_case(k, n) with its exclusions, and the gallery's
    max ||g||^2."""
    g, q, glab, plab, excl = random_case(k, n)
    s = lu.score_matrix(q, g, metric)
    return {rel: lu.top2_masked(q, g, metric, glab, plab, rel, excl, s=s) for rel in RELATIONS}, pu.gmax2_of(g)


PEOPLE, PER = 10, 150


@functools.lru_cache(maxsize=None)
def loo_case(k, seed=11):
    """Test 4's person-by-person gallery: 10 people x 150 rows around well separated centres,
    with planted identical rows inside a person and across two people."""
    rng = np.random.default_rng(seed + k)
    d = rng.standard_normal(k)
    m = d / np.linalg.norm(d) * 12.0 * np.sqrt(k)
    centres = m + 4.0 * rng.standard_normal((PEOPLE, k))
    rows = (centres[:, None, :] + 0.3 * rng.standard_normal((PEOPLE, PER, k))).reshape(PEOPLE * PER, k)
    g = rows.astype(np.float32)
    labels = np.repeat(np.arange(PEOPLE), PER).astype(np.int32)
    for p in range(PEOPLE):
        b0 = p * PER
        g[[b0, b0 + 1, b0 + 2]] = (-m + 4.0 * rng.standard_normal(k)).astype(np.float32)
        if p % 2 == 0:
            g[[b0 + 3, b0 + 153, b0 + 154]] = (-m + 4.0 * rng.standard_normal(k)).astype(np.float32)
            g[b0 + 157] = g[b0 + 7]
    return g, labels


@functools.lru_cache(maxsize=None)
def loo_refs(k, metric):
    g, labels = loo_case(k)
    n = len(g)
    s = lu.score_matrix(g, g, metric)
    rows = np.arange(n)
    return {rel: lu.top2_masked(g, g, metric, labels, labels, rel, rows, s=s) for rel in ("same", "other")}, pu.gmax2_of(g)


@functools.lru_cache(maxsize=None)
def near_tie_case(k, metric, n=5003):
    """Test 5: two labels; every probe's fp64 SAME answer gets a rival a few ulps away (plant_rivals),
    labelled like the probe for even probes and with the other label for odd ones."""
    rng = np.random.default_rng(77 + k)
    g0 = rng.standard_normal((n, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    glab = rng.integers(0, 2, n).astype(np.int32)
    plab = rng.integers(0, 2, B).astype(np.int32)
    anchors = lu.top2_masked(q, g0, metric, glab, plab, "same")[0]
    G, rivals = pu.plant_rivals(g0, q, anchors, seed=5)
    glab = glab.copy()
    even = np.arange(B) % 2 == 0
    glab[rivals] = np.where(even, plab, 1 - plab)
    return G, q, glab, plab, rivals
