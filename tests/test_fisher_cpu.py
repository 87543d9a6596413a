"""Host half of the Fisher discriminant (no GPU): the stable grouping ef_lda_order, the fold of
the discriminant into a projection matrix, the estimator's file format, and the host reference
of the GPU tests pinned to sklearn."""
import numpy as np
import pytest

import fisher_util as fu


def _order(labels, n_classes, pad=8):
    """ef_lda_order on guarded arrays: (rc, order, offsets); the guards around both outputs
    must come back untouched."""
    from eigenface import _native
    lib = _native.lib()
    lab = np.ascontiguousarray(labels, dtype=np.int32)
    n = lab.size
    order = np.full(n + 2 * pad, -7, np.int64)
    offsets = np.full(n_classes + 1 + 2 * pad, -7, np.int64)
    rc = lib.ef_lda_order(lab.ctypes.data, n, n_classes, order[pad:].ctypes.data, offsets[pad:].ctypes.data)
    for a in (order, offsets):
        assert (a[:pad] == -7).all() and (a[len(a) - pad:] == -7).all()
    return rc, order[pad:pad + n], offsets[pad:pad + n_classes + 1]


def test_lda_symbols_are_bound():
    from eigenface import _native
    lib = _native.lib()
    for name in ("ef_lda_order", "ef_lda_scatter", "ef_lda_fit"):
        assert hasattr(lib, name) and name in _native.EXPORTED_SYMBOLS
    assert lib.ef_api_version() == 7


@pytest.mark.parametrize("labels,n_classes", [
    (np.arange(9000) % 3000, 3000),                                  # interleaved
    (np.array([4, 0, 4, 2, 0, 4, 2, 2, 0]), 6),                      # classes 1, 3, 5 empty
    (np.zeros(17, np.int32), 1),                                     # C = 1
    (np.zeros(0, np.int32), 3),                                      # n = 0
    (np.random.default_rng(3).integers(0, 37, 20011), 37),
])
def test_lda_order_is_the_stable_grouping(labels, n_classes):
    rc, order, offsets = _order(labels, n_classes)
    assert rc == 0
    np.testing.assert_array_equal(order, np.argsort(labels, kind="stable"))
    np.testing.assert_array_equal(np.diff(offsets), np.bincount(labels, minlength=n_classes))
    assert offsets[0] == 0 and offsets[-1] == len(labels)


@pytest.mark.parametrize("bad", [5, -1, 2 ** 31 - 1, -2 ** 31])
def test_lda_order_refuses_a_label_out_of_range(bad):
    from eigenface import _native
    labels = np.array([0, 3, bad, 4, 1], np.int64).astype(np.int32)
    rc, order, offsets = _order(labels, 5)
    assert rc == _native.EF_E_INVALID
    assert (order == -7).all() and (offsets == -7).all()  # nothing written at all


def test_fold_is_the_fp64_product():
    from eigenface.fisher import fold_scalings
    rng = np.random.default_rng(0)
    W = rng.standard_normal((576, 32)).astype(np.float32)  # a model's float32 W folds in float64 too
    A = rng.standard_normal((32, 9))
    Wf = fold_scalings(W, A)
    assert Wf.dtype == np.float64
    np.testing.assert_array_equal(Wf, W.astype(np.float64) @ A)
    with pytest.raises(ValueError):
        fold_scalings(W, A[:-1])


def test_pca_width_rule():
    from eigenface.fisher import pca_components_for
    assert pca_components_for(300, 10) == 256
    assert pca_components_for(300, 10, 32) == 32
    assert pca_components_for(100, 10) == 90
    assert pca_components_for(100, 10, 500) == 90
    with pytest.raises(ValueError):
        pca_components_for(10, 10)


def test_save_load_round_trip_is_byte_equal(tmp_path):
    from eigenface import Fisherfaces
    rng = np.random.default_rng(1)
    f = Fisherfaces(n_components=4)
    f.labels_ = rng.integers(0, 5, 40).astype(np.int32)
    f.classes_ = np.array(["ann", "bob", "cy", "di", "ed"])
    f.eigenvalues_ = np.sort(rng.random(4))[::-1].copy()
    f.n_components_ = 4
    f._set_model(rng.random(64), rng.standard_normal((64, 4)), rng.standard_normal((40, 4)))
    path = f.save(str(tmp_path / "fisher.npz"))
    g = Fisherfaces.load(path)
    for name in ("mean_", "scalings_", "face_features_", "labels_", "classes_", "eigenvalues_", "_W", "_mu"):
        a, b = getattr(f, name), getattr(g, name)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert g.n_components_ == 4 and not hasattr(g, "inverse_transform")
    # a second save of the loaded estimator writes the same arrays again
    with np.load(g.save(str(tmp_path / "again.npz"))) as z, np.load(path) as z0:
        assert sorted(z.files) == sorted(z0.files)
        for k in z.files:
            assert z[k].tobytes() == z0[k].tobytes()


def test_reference_separates_the_lighting_case():
    """The host reference on the lighting case: the discriminant features are recognised
    leave-one-out, the raw features are not (nearest other row by L2, on the host)."""
    c = fu.fit_case("lighting")
    F, lab = c["F"], c["labels"]

    def rank1(x):
        d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(d, np.inf)
        return float((lab[d.argmin(1)] == lab).mean())

    assert c["cond"] <= 1e6
    assert rank1(F) <= 0.5
    assert rank1(F @ c["ref_A"][:, :c["m"]]) == 1.0


def test_reference_matches_sklearn_span():
    pytest.importorskip("sklearn")
    from sklearn.discriminant_analysis import LinearDiscriminantAnalysis
    c = fu.fit_case("lighting")
    m = c["C"] - 1
    sk = LinearDiscriminantAnalysis(solver="eigen").fit(c["F"], c["labels"]).scalings_[:, :m]
    ref = c["ref_A"][:, :m]
    coef = np.linalg.lstsq(ref, sk, rcond=None)[0]
    res = np.linalg.norm(sk - ref @ coef, axis=0) / np.linalg.norm(sk, axis=0)
    assert res.max() < 1e-10, res.max()  # measured below 1e-13
