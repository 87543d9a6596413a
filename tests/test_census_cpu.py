"""Host half of the score census: rates, equal error, TAR at FMR, AUC and d' from hand-built
(2, nbins + 3) counts, and the input checks of Engine.score_census (no GPU needed)."""
import ctypes

import numpy as np
import pytest


def _counts(nbins, genuine=(), impostor=()):
    """counts from {slot: count} per side."""
    c = np.zeros((2, nbins + 3), np.int64)
    for side, d in enumerate((dict(genuine), dict(impostor))):
        for slot, v in d.items():
            c[side, slot] = v
    return c


def test_names_are_exported():
    import eigenface
    for name in ("score_census", "verification_rates", "VerificationRates", "pair_equal_error", "tar_at_fmr", "auc",
                 "d_prime", "compare_verification"):
        assert hasattr(eigenface, name) and name in eigenface.__all__


def test_hand_worked_rates_both_directions():
    from eigenface import verification_rates
    # 4 bins over (0, 4): edges 0 1 2 3 4.  genuine: 1 below, bins (2, 1, 0, 0), 0 over;
    # impostor: 0 below, bins (0, 1, 2, 0), 1 over
    c = _counts(4, {0: 1, 1: 2, 2: 1}, {2: 1, 3: 2, 5: 1})
    r = verification_rates(c, 0.0, 4.0, "l2")  # accept: binned below the edge
    np.testing.assert_array_equal(r.thresholds, [0, 1, 2, 3, 4])
    np.testing.assert_allclose(r.fmr, [0, 0, 0.25, 0.75, 0.75])
    np.testing.assert_allclose(r.fnmr, [0.75, 0.25, 0, 0, 0])
    assert (r.n_genuine, r.n_impostor, r.nonfinite, r.metric) == (4, 4, (0, 0), "l2")
    r = verification_rates(c, 0.0, 4.0, "cosine")  # accept: binned at or above the edge
    np.testing.assert_allclose(r.fmr, [1, 1, 0.75, 0.25, 0.25])
    np.testing.assert_allclose(r.fnmr, [0.25, 0.75, 1, 1, 1])


def test_separated_distributions():
    from eigenface import auc, d_prime, pair_equal_error, tar_at_fmr, verification_rates
    # cosine: impostors in bins 0 - 1, genuine in bins 6 - 7 of 8 over (-1, 1)
    c = _counts(8, {7: 30, 8: 70}, {1: 500, 2: 500})
    r = verification_rates(c, -1.0, 1.0, "cosine")
    t, eer = pair_equal_error(r)
    assert eer == 0.0 and t == 0.5  # the strictest of the edges -0.5 .. 0.5 that separate: the largest similarity
    assert auc(r) == 1.0 and tar_at_fmr(r, 1e-3) == 1.0 and tar_at_fmr(r, 0.0) == 1.0
    # L2: genuine low, impostor high; the strictest separating edge is the smallest distance
    c = _counts(8, {1: 30, 2: 70}, {7: 500, 8: 500})
    r = verification_rates(c, 0.0, 8.0, "l2")
    assert pair_equal_error(r) == (2.0, 0.0) and auc(r) == 1.0 and tar_at_fmr(r, 1e-3) == 1.0
    # d': centres 0.5 (30) and 1.5 (70) against 6.5 and 7.5 (500 each)
    mg, mi = 0.3 * 0.5 + 0.7 * 1.5, 7.0
    vg, vi = 0.3 * (0.5 - mg) ** 2 + 0.7 * (1.5 - mg) ** 2, 0.25
    assert d_prime(c, 0.0, 8.0) == pytest.approx((mi - mg) / np.sqrt((vg + vi) / 2), rel=1e-12)


def test_identical_distributions():
    from eigenface import auc, d_prime, pair_equal_error, verification_rates
    hist = {1: 10, 2: 40, 3: 40, 4: 10}
    for metric in ("cosine", "l2"):
        r = verification_rates(_counts(4, hist, {k: 3 * v for k, v in hist.items()}), -1.0, 1.0, metric)
        np.testing.assert_allclose(r.fmr + r.fnmr, 1.0)
        t, eer = pair_equal_error(r)
        assert (t, eer) == (0.0, 0.5)
        assert auc(r) == pytest.approx(0.5, abs=1e-15)
    assert d_prime(_counts(4, hist, hist), -1.0, 1.0) == 0.0


def test_empty_side_and_non_finite_slot():
    from eigenface import auc, d_prime, pair_equal_error, tar_at_fmr, verification_rates
    # the non-finite slot is in no denominator: 4 finite genuine pairs of 4 + 96
    c = _counts(4, {1: 2, 4: 2, 6: 96}, {2: 5, 3: 5, 6: 1000})
    r = verification_rates(c, 0.0, 4.0, "l2")
    assert (r.n_genuine, r.n_impostor, r.nonfinite) == (4, 10, (96, 1000))
    np.testing.assert_allclose(r.fnmr, [1, 0.5, 0.5, 0.5, 0])
    np.testing.assert_allclose(r.fmr, [0, 0, 0.5, 1, 1])
    # no impostor pair at all (a one-class gallery): FMR is NaN and does not count
    r = verification_rates(_counts(4, {1: 2, 4: 2}, {6: 7}), 0.0, 4.0, "l2")
    assert np.isnan(r.fmr).all() and not np.isnan(r.fnmr).any()
    assert pair_equal_error(r) == (4.0, 0.0)
    assert np.isnan(auc(r)) and np.isnan(tar_at_fmr(r, 0.5)) and np.isnan(d_prime(_counts(4, {1: 2}, {6: 7}), 0.0, 4.0))
    r = verification_rates(_counts(4), 0.0, 4.0, "cosine")
    t, eer = pair_equal_error(r)
    assert np.isnan(t) and np.isnan(eer) and np.isnan(r.fnmr).all()
    # outer slots have no centre: d' ignores them
    assert d_prime(_counts(4, {0: 50, 1: 3, 5: 9}, {4: 3, 5: 70}), 0.0, 4.0) == np.inf


def test_tar_at_fmr_boundary():
    from eigenface import tar_at_fmr, verification_rates
    c = _counts(4, {1: 1, 2: 1, 3: 1, 4: 1}, {2: 1, 3: 1, 4: 2})
    r = verification_rates(c, 0.0, 4.0, "l2")
    np.testing.assert_allclose(r.fmr, [0, 0, 0.25, 0.5, 1])
    np.testing.assert_allclose(1 - r.fnmr, [0, 0.25, 0.5, 0.75, 1])
    assert tar_at_fmr(r, 0.25) == 0.5       # an FMR equal to the target qualifies
    assert tar_at_fmr(r, 0.2499) == 0.25
    assert tar_at_fmr(r, 0.0) == 0.25 and tar_at_fmr(r, 1.0) == 1.0
    assert np.isnan(tar_at_fmr(r, -0.1))    # no edge qualifies


def test_host_functions_check_their_input():
    from eigenface import d_prime, verification_rates
    good = _counts(4, {1: 1}, {2: 1})
    for bad in (np.zeros((3, 7), np.int64), np.zeros(7, np.int64), np.zeros((2, 3), np.int64), good.astype(np.float64),
                -good):
        with pytest.raises(ValueError):
            verification_rates(bad, 0.0, 1.0, "l2")
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, float("nan")), (0.0, float("inf"))):
        with pytest.raises(ValueError):
            verification_rates(good, lo, hi, "l2")
        with pytest.raises(ValueError):
            d_prime(good, lo, hi)
    with pytest.raises(ValueError):
        verification_rates(good, 0.0, 1.0, "dot")


def _hostless_engine(gallery_k=None):
    """An Engine whose context was never created (the pattern of test_native_abi): the input
    checks run before any C call, which would fail on the NULL context."""
    from eigenface import Engine, _native
    e = object.__new__(Engine)
    e._lib = _native.lib()
    e._h = ctypes.c_void_p()
    e.model_d, e.model_k, e.gallery_k, e.gallery_n = None, None, gallery_k, 0
    return e


def test_engine_census_checks_inputs_before_the_c_call():
    q, lab = np.zeros((4, 8), np.float32), np.zeros(4, np.int32)
    with pytest.raises(RuntimeError):
        _hostless_engine().score_census(q, lab)
    e = _hostless_engine(gallery_k=8)
    for bad_q in (np.zeros((4, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 2, 8), np.float32)):
        with pytest.raises(ValueError):
            e.score_census(bad_q, lab)
    for kw in (dict(nbins=0), dict(nbins=2049), dict(range=(1.0, 1.0)), dict(range=(1.0, -1.0)),
               dict(range=(float("nan"), 1.0)), dict(range=(0.0, float("inf"))), dict(range=(0.0, 1e-46)),
               dict(exclude_rows=np.zeros(3, np.int64)), dict(exclude_rows=np.zeros((4, 1), np.int64)),
               dict(counts=np.zeros((2, 259), np.int64))):
        with pytest.raises(ValueError):
            e.score_census(q, lab, **kw)
    for bad_lab in (None, np.zeros(3, np.int32), np.zeros((4, 1), np.int32)):
        with pytest.raises(ValueError):
            e.score_census(q, bad_lab)


def test_library_exports_the_census():
    from eigenface import _native
    assert "ef_score_census" in _native.EXPORTED_SYMBOLS
    lib = _native.lib()
    assert lib.ef_api_version() == 7
    # a NULL context is refused before anything else is read
    assert lib.ef_score_census(None, None, 0, 0, None, None, 0.0, 1.0, 4, None, 0) == _native.EF_E_INVALID
