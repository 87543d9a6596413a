"""CPU-side checks of the reconstruction feature: the library exports it, the fp64 yardstick of
tests/recon_util.py is itself pinned against sklearn, and the R / s derivation inverts W."""
import numpy as np

import recon_util as ru


def test_library_exports_reconstruction_symbols():
    from eigenface import _native
    lib = _native.lib()
    for n in ("ef_recon_set", "ef_reconstruct", "ef_face_distance"):
        assert n in _native.EXPORTED_SYMBOLS, n
        assert hasattr(lib, n), n


def _sklearn_pair(rng, n, d, k):
    from sklearn.decomposition import PCA
    from sklearn.preprocessing import StandardScaler
    x = rng.integers(0, 256, (n, d)).astype(np.float64)
    x[:, 3] = 7.0  # a constant pixel: the scaler's scale is 1 there
    sc = StandardScaler().fit(x)
    pca = PCA(n_components=k, svd_solver="full").fit(sc.transform(x))
    return x, sc, pca


def test_reference_agrees_with_sklearn_chain():
    rng = np.random.default_rng(5)
    x, sc, pca = _sklearn_pair(rng, 40, 96, 6)
    W, R, s = ru.standardised_operands(pca.components_, sc.scale_)
    mean = sc.mean_ + sc.scale_ * pca.mean_
    f = pca.transform(sc.transform(x))
    np.testing.assert_allclose((x - mean) @ W, f, rtol=0, atol=1e-11 * np.abs(f).max())
    want = sc.inverse_transform(pca.inverse_transform(f))
    got = ru.reconstruct_ref(f, R, mean)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())
    # the residual, directly: in the scaler's space, where the components are orthonormal
    z = sc.transform(x)
    direct = ((z - pca.inverse_transform(f)) ** 2).sum(axis=1)
    r = ru.residual_ref(x, f, R, mean, s)
    np.testing.assert_allclose((r * r).sum(axis=1), direct, rtol=1e-10)
    e = ru.centred_ref(x, mean, s)
    np.testing.assert_allclose((e * e).sum(axis=1), ((z - pca.mean_) ** 2).sum(axis=1), rtol=1e-10)
    # orthonormal basis: Pythagoras holds for the reference (the kernel never relies on it)
    np.testing.assert_allclose((r * r).sum(axis=1), (e * e).sum(axis=1) - (f * f).sum(axis=1), rtol=1e-8)


def test_standardised_operands_invert_the_projection():
    rng = np.random.default_rng(6)
    d, k = 200, 9
    V = ru.orthonormal_rows(rng, k, d)
    sigma = rng.uniform(0.5, 60.0, d)
    sigma[[0, 17]] = 0.0  # the scaler's rule: a zero scale counts as 1
    W, R, s = ru.standardised_operands(V, sigma)
    f = rng.standard_normal((11, k)) * 40.0
    back = (f @ R) @ W  # (x^ - mean) . W
    assert np.abs(back - f).max() <= 1e-12 * np.abs(f).max()
    assert s[0] == 1.0 and s[17] == 1.0
    # the package's fp32 operands are this derivation, rounded once
    from eigenface.pca import reconstruction_operands
    R32, s32 = reconstruction_operands(V, sigma)
    np.testing.assert_array_equal(R32, R.astype(np.float32))
    np.testing.assert_array_equal(s32, s.astype(np.float32))
    R0, s0 = reconstruction_operands(V, None)
    np.testing.assert_array_equal(R0, V.astype(np.float32))
    assert s0 is None


def test_u8_rule_and_undecided_pixels():
    x = np.array([[-3.0, -0.4, 0.5, 1.5, 2.5, 254.5, 255.4, 255.6, 300.0, 100.2, 0.49999]])
    np.testing.assert_array_equal(ru.u8_ref(x), [[0, 0, 0, 2, 2, 254, 255, 255, 255, 100, 0]])
    und = ru.u8_undecided(x, np.full(x.shape, 1e-4))
    np.testing.assert_array_equal(und, [[False, False, True, True, True, True, False, False, False, False, True]])
