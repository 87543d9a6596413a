"""The labelled search's guarantee as test assertions: per probe, exactly what parity_util
asserts of the plain search, on the sub-gallery of qualifying rows.

A row qualifies when its label stands in the relation to the probe's ("same", "other", "any")
and its index is not the probe's excluded row (a negative entry excludes nothing).  Scores are
fp64, 'smaller is better', in parity_util.top2's forms: expanded L2, unit-row dot products for
cosine.  The window and margin are parity_util's, with the scale of the WHOLE gallery.
"""
import numpy as np

import parity_util as pu
from oracle import eigenface_oracle as orc


def score_matrix(q, g, metric):
    q64, g64 = np.asarray(q, np.float64), np.asarray(g, np.float64)
    if metric == "l2":
        return (q64 ** 2).sum(1)[:, None] + (g64 ** 2).sum(1)[None, :] - 2.0 * (q64 @ g64.T)
    return -(orc._unit_rows(q64) @ orc._unit_rows(g64).T)


def qualifies(glab, plab, relation, excl, n):
    """(b, n) bool: row r qualifies for probe p."""
    b = len(plab) if plab is not None else len(excl)
    if relation == "any":
        ok = np.ones((b, n), bool)
    else:
        eq = np.asarray(glab)[None, :] == np.asarray(plab)[:, None]
        ok = eq if relation == "same" else ~eq
    if excl is not None:
        e = np.asarray(excl, np.int64)
        has = (e >= 0) & (e < n)
        ok = ok.copy()
        ok[np.flatnonzero(has), e[has]] = False
    return ok


def top2_masked(q, g, metric, glab, plab, relation, excl=None, s=None):
    """(first best qualifying row or -1, best, runner-up among the qualifying rows)."""
    s = score_matrix(q, g, metric) if s is None else s
    b, n = s.shape
    if plab is None and excl is None:
        ok = np.ones((b, n), bool)
    else:
        ok = qualifies(glab, plab, relation, excl, n)
    m = np.where(ok, s, np.inf)
    idx = np.argmin(m, axis=1)  # first minimum
    best = m[np.arange(b), idx]
    m[np.arange(b), idx] = np.inf
    second = m.min(axis=1) if n > 1 else np.full(b, np.inf)
    idx = np.where(np.isfinite(best), idx, -1)
    return idx, best, second, s, ok


def clear_mask(q, g, metric, ref, gmax2=None):
    """Probes whose qualifying top-2 gap exceeds 1.1 x the window (those without a qualifying
    row count as clear: their answer, 'none', is exact)."""
    idx, best, second = ref[:3]
    w = pu.MARGIN * pu.window(q, g, metric, np.where(idx >= 0, best, 0.0), gmax2)
    with np.errstate(invalid="ignore"):  # inf - inf where no row qualifies
        return (idx < 0) | ((second - best) > w), w


def assert_labelled(q, g, metric, got_idx, ref, gmax2=None):
    """The guarantee: the exact row where the qualifying top-2 gap exceeds 1.1 x window, a row
    inside the window otherwise, -1 exactly where no row qualifies.  Returns the clear mask."""
    idx, best, second, s, ok = ref
    got = np.asarray(got_idx)
    none = idx < 0
    np.testing.assert_array_equal(got < 0, none, err_msg=f"{metric}: 'no qualifying row' differs")
    clear, w = clear_mask(q, g, metric, ref, gmax2)
    have = ~none
    assert ok[np.flatnonzero(have), got[have]].all(), f"{metric}: a returned row does not qualify"
    mine = s[np.flatnonzero(have), got[have]]
    bad = ~(mine - best[have] <= w[have])
    assert not bad.any(), f"{metric}: {bad.sum()} probes chose a row outside the tie window " \
                          f"(first {np.flatnonzero(have)[bad][:5]})"
    miss = clear & (got != idx)
    assert not miss.any(), f"{metric}: {miss.sum()} of {clear.sum()} clear probes differ from the fp64 " \
                           f"first-arg-best (first {np.flatnonzero(miss)[:5]})"
    return clear
