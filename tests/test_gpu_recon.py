"""Reconstruction and distance from face space on the GPU (ef_recon_set, ef_reconstruct,
ef_face_distance) against the fp64 reference and the bounds of tests/recon_util.py.

The residual's reference is evaluated at the engine's own returned features, which isolates the
back-projection from the projection's own, separately tested, error; one end-to-end case runs the
whole fp64 pipeline with the projection's bound carried through |R|.
"""
import numpy as np
import pytest

import recon_util as ru

pytestmark = pytest.mark.gpu

# ragged tiles in b and d, d % 16 != 0, k = 1, a k that is no tile multiple, k beyond one 512 slice
SHAPES = [(333, 10), (4096, 1), (4096, 50), (10000, 200), (4096, 640)]
BS = [1, 129, 300]
EF_E_INVALID, EF_E_STATE = -1, -3


@pytest.fixture(scope="module")
def eng():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from eigenface import Engine
    e = Engine(0)
    yield e
    e.close()


_models = {}


def _model(d, k, weighted):
    """(mean, W (d, k), R (k, d), s or None) as fp32, built once per shape: orthonormal rows V,
    and with a weight s ~ U(0.02, 1) the standardised form W = diag(s) V^T, R = V diag(1/s)."""
    key = (d, k, weighted)
    if key not in _models:
        rng = np.random.default_rng(1000 * d + 10 * k + weighted)
        V = ru.orthonormal_rows(rng, k, d)
        mean = rng.uniform(100.0, 156.0, d).astype(np.float32)
        if weighted:
            s = rng.uniform(0.02, 1.0, d)
            W, R, s = ru.standardised_operands(V, 1.0 / s)
            s = s.astype(np.float32)
        else:
            W, R, s = V.T, V, None
        _models[key] = (mean, np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(R, dtype=np.float32), s)
    return _models[key]


def _load(eng, d, k, weighted, precision="fp32"):
    mean, W, R, s = _model(d, k, weighted)
    eng.set_model(mean, W, precision=precision)
    eng.set_reconstruction(R, s)
    return mean, W, R, s


def _pixels(kind, rng, b, mean, R, s):
    d, k = mean.shape[0], R.shape[0]
    if kind == "random":
        return rng.integers(0, 256, (b, d), dtype=np.uint8)
    # near face space: p = rint(mean + f0 . R), f0 ~ N(0, 15^2 d / k) (about +-15 grey levels per
    # pixel over orthonormal rows); with a weight, R = V diag(1/s) is up to 50 times larger, so f0
    # is scaled by min(s) to stay inside the uint8 range
    amp = 15.0 * np.sqrt(d / k) * (1.0 if s is None else float(s.min()))
    f0 = rng.standard_normal((b, k)) * amp
    return np.clip(np.rint(ru.reconstruct_ref(f0, R, mean)), 0, 255).astype(np.uint8)


def _check_distance(P, mean, R, s, F, eps2, energy, k, what, extra=None, F_ref=None):
    d = mean.shape[0]
    Fr = F if F_ref is None else F_ref
    r = ru.residual_ref(P, Fr, R, mean, s)
    e = ru.residual_err(P, Fr, R, mean, s, extra)
    ref = (r * r).sum(axis=1)
    bound = ru.sumsq_bound(r, e, d + k)
    err = np.abs(ru.f64(eps2) - ref)
    print(f"{what}: eps2 ref {ref.min():.6g}..{ref.max():.6g}  max err/bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound), (what, float(np.max(err / bound)))
    if energy is not None:
        c = ru.centred_ref(P, mean, s)
        ec = ru.residual_err(P, np.zeros_like(ru.f64(Fr)), R, mean, s)
        eref = (c * c).sum(axis=1)
        eb = ru.sumsq_bound(c, ec, d + k)
        eerr = np.abs(ru.f64(energy) - eref)
        print(f"{what}: eps2 / E {np.median(ref / eref):.3g}  max err/bound {np.max(eerr / eb):.3g}")
        assert np.all(eerr <= eb), (what, float(np.max(eerr / eb)))


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("d,k", SHAPES)
def test_face_distance_u8(eng, d, k, b):
    for weighted in (False, True):
        mean, W, R, s = _load(eng, d, k, weighted)
        for kind in ("random", "near"):
            rng = np.random.default_rng(d + k + b + weighted)
            P = _pixels(kind, rng, b, mean, R, s)
            eps2, energy, F = eng.face_distance(P, return_energy=True, return_features=True)
            assert eps2.shape == (b,) and energy.shape == (b,) and F.shape == (b, k)
            np.testing.assert_array_equal(F, eng.project(P))  # bit-equal: the same projection
            np.testing.assert_array_equal(eng.face_distance(P), eps2)  # with and without the optional outputs
            _check_distance(P, mean, R, s, F, eps2, energy, k, f"d={d} k={k} b={b} w={weighted} {kind}")


def test_face_distance_f32_pixels(eng):
    d, k, b = 4096, 50, 129
    mean, W, R, s = _load(eng, d, k, True)
    rng = np.random.default_rng(7)
    P = (rng.uniform(0, 255, (b, d))).astype(np.float32)
    eps2, energy, F = eng.face_distance(P, return_energy=True, return_features=True)
    np.testing.assert_array_equal(F, eng.project(P))
    _check_distance(P, mean, R, s, F, eps2, energy, k, "f32 pixels")
    # rows that are not 16-byte aligned take the per-pixel loads
    d2, k2 = 333, 10
    mean, W, R, s = _load(eng, d2, k2, True)
    P = (rng.uniform(0, 255, (b, d2))).astype(np.float32)
    eps2, energy, F = eng.face_distance(P, return_energy=True, return_features=True)
    _check_distance(P, mean, R, s, F, eps2, energy, k2, "f32 pixels, d=333")


def test_face_distance_bf16_model(eng):
    """The bf16 model's features carry about 1e-3 of error; the back-projection is fp32, so the
    bound at the returned features is the fp32 one."""
    d, k, b = 4096, 50, 129
    mean, W, R, s = _load(eng, d, k, False, precision="bf16")
    rng = np.random.default_rng(8)
    for kind in ("random", "near"):
        P = _pixels(kind, rng, b, mean, R, s)
        eps2, energy, F = eng.face_distance(P, return_energy=True, return_features=True)
        np.testing.assert_array_equal(F, eng.project(P))
        _check_distance(P, mean, R, s, F, eps2, energy, k, f"bf16 model {kind}")


def _recon_features(rng, b, d, k):
    return (25.0 * np.sqrt(d) * rng.standard_normal((b, k))).astype(np.float32)


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("d,k", SHAPES)
def test_reconstruct_f32(eng, d, k, b):
    mean, W, R, s = _load(eng, d, k, False)
    F = _recon_features(np.random.default_rng(d + k + b), b, d, k)
    got = eng.reconstruct(F)
    assert got.dtype == np.float32 and got.shape == (b, d)
    ref = ru.reconstruct_ref(F, R, mean)
    tol = ru.recon_err(F, R, mean)
    err = np.abs(ru.f64(got) - ref)
    out = np.mean((ref < 0) | (ref > 255))
    print(f"d={d} k={k} b={b}: outside [0, 255] {100 * out:.1f} %  max err/bound {np.max(err / tol):.3g}")
    assert np.all(err <= tol), float(np.max(err / tol))


def _check_u8(got, F, R, mean, what):
    ref = ru.reconstruct_ref(F, R, mean)
    und = ru.u8_undecided(ref, ru.recon_err(F, R, mean))
    share = float(und.mean())
    print(f"{what}: undecided {100 * share:.3f} %")
    assert share <= 0.01, (what, share)  # a case that excludes more than 1 % fails
    want = ru.u8_ref(ref)
    bad = (got != want) & ~und
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4], ref[bad][:4])


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("d,k", SHAPES)
def test_reconstruct_u8(eng, d, k, b):
    mean, W, R, s = _load(eng, d, k, False)
    rng = np.random.default_rng(d + k + b + 1)
    F = _recon_features(rng, b, d, k)
    got = eng.reconstruct(F, "uint8")
    assert got.dtype == np.uint8 and got.shape == (b, d)
    _check_u8(got, F, R, mean, f"d={d} k={k} b={b}")
    # features of random pixels: the reconstruction stays inside the range
    F = eng.project(rng.integers(0, 256, (b, d), dtype=np.uint8))
    _check_u8(eng.reconstruct(F, "uint8"), F, R, mean, f"d={d} k={k} b={b} (random pixels)")


def test_end_to_end_fp64_pipeline(eng):
    """fp64 projection of the fp32-stored mean and W, then the fp64 residual; the projection's
    |df| <= 2e-6 (|p - mean| . |W|) + 1e-6 goes through |R| into the per-pixel error."""
    d, k, b = 4096, 50, 129
    for weighted in (False, True):
        mean, W, R, s = _load(eng, d, k, weighted)
        rng = np.random.default_rng(9 + weighted)
        for kind in ("random", "near"):
            P = _pixels(kind, rng, b, mean, R, s)
            eps2 = eng.face_distance(P)
            c = ru.centred_ref(P, mean)
            F64 = c @ ru.f64(W)
            dF = 2e-6 * (np.abs(c) @ np.abs(ru.f64(W))) + 1e-6
            extra = dF @ np.abs(ru.f64(R))
            _check_distance(P, mean, R, s, None, eps2, None, k, f"e2e w={weighted} {kind}", extra=extra, F_ref=F64)


def test_deterministic(eng):
    d, k, b = 10000, 200, 300  # the pixel axis is split over workgroups here
    mean, W, R, s = _load(eng, d, k, True)
    P = np.random.default_rng(10).integers(0, 256, (b, d), dtype=np.uint8)
    a1, e1 = eng.face_distance(P, return_energy=True)
    a2, e2 = eng.face_distance(P, return_energy=True)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(e1, e2)
    assert np.all(a1 > 0)
    # the two kernels have timers of their own: one launch each per call
    eng.timing_reset()
    eng.timing(True)
    try:
        eng.face_distance(P)
        (ms, n), (ms2, n2) = eng.timing_get("recon"), eng.timing_get("recon_reduce")
        assert n == 1 and n2 == 1 and ms > 0 and ms2 > 0
    finally:
        eng.timing(False)
        eng.timing_reset()


def test_device_tensors(eng):
    import torch
    d, k, b = 4096, 50, 129
    mean, W, R, s = _load(eng, d, k, True)
    rng = np.random.default_rng(11)
    P = rng.integers(0, 256, (b, d), dtype=np.uint8)
    h_eps, h_en, h_f = eng.face_distance(P, return_energy=True, return_features=True)
    dev = torch.device("cuda", eng.device)
    out = torch.full((b,), -1.0, dtype=torch.float32, device=dev)
    t_eps, t_en, t_f = eng.face_distance(torch.from_numpy(P).to(dev), return_energy=True, return_features=True,
                                         out=out)
    assert t_eps is out
    eng.synchronize()
    np.testing.assert_array_equal(t_eps.cpu().numpy(), h_eps)
    np.testing.assert_array_equal(t_en.cpu().numpy(), h_en)
    np.testing.assert_array_equal(t_f.cpu().numpy(), h_f)
    F = _recon_features(rng, b, d, k)
    for dtype, tdt in (("float32", torch.float32), ("uint8", torch.uint8)):
        want = eng.reconstruct(F, dtype)
        out = torch.zeros((b, d), dtype=tdt, device=dev)
        got = eng.reconstruct(torch.from_numpy(F).to(dev), dtype, out=out)
        assert got is out
        eng.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), want)
    # device operands of set_reconstruction give the same state
    eng.set_reconstruction(torch.from_numpy(R).to(dev), torch.from_numpy(s).to(dev))
    np.testing.assert_array_equal(eng.face_distance(P), h_eps)
    with pytest.raises(ValueError):
        eng.reconstruct(torch.from_numpy(F).to(dev), "float32", out=torch.zeros((b, d + 1), device=dev))


def test_state_rules():
    from eigenface import EigenfaceError, Engine
    d, k = 333, 10
    mean, W, R, s = _model(d, k, True)
    P = np.random.default_rng(12).integers(0, 256, (5, d), dtype=np.uint8)
    F = np.zeros((5, k), np.float32)
    with Engine(0) as e:
        with pytest.raises(RuntimeError):
            e.set_reconstruction(R, s)  # no model at all
        e.set_model(mean, W)
        for call in (lambda: e.face_distance(P), lambda: e.reconstruct(F)):
            with pytest.raises(EigenfaceError) as ei:
                call()
            assert ei.value.code == EF_E_STATE
        for badR, bads in ((R[:, :-1], s[:-1]), (R[:-1], s)):  # d, then k, differ from the model's
            with pytest.raises(EigenfaceError) as ei:
                e.set_reconstruction(badR, bads)
            assert ei.value.code == EF_E_INVALID
        f0 = e.project(P)  # the model is still usable
        assert f0.shape == (5, k)
        with pytest.raises(EigenfaceError) as ei:  # and the failed call left no reconstruction state
            e.face_distance(P)
        assert ei.value.code == EF_E_STATE
        e.set_reconstruction(R, s)
        eps2 = e.face_distance(P)
        assert eps2.shape == (5,) and np.all(np.isfinite(eps2))
        np.testing.assert_array_equal(e.project(P), f0)
        # b = 0: empty results, no error
        z = e.face_distance(P[:0], return_energy=True, return_features=True)
        assert [a.shape for a in z] == [(0,), (0,), (0, k)]
        assert e.reconstruct(F[:0]).shape == (0, d) and e.reconstruct(F[:0], "uint8").dtype == np.uint8
        with pytest.raises(ValueError):
            e.reconstruct(F, "float16")
        with pytest.raises(ValueError):
            e.reconstruct(F[:, :-1])
        # a new model drops the reconstruction state
        e.set_model(mean, W)
        for call in (lambda: e.face_distance(P), lambda: e.reconstruct(F)):
            with pytest.raises(EigenfaceError) as ei:
                call()
            assert ei.value.code == EF_E_STATE


@pytest.fixture(scope="module")
def synth():
    rng = np.random.default_rng(13)
    n, d = 60, 1024
    basis = rng.standard_normal((12, d))
    x = 128.0 + 6.0 * rng.standard_normal((n, 12)) @ basis + 3.0 * rng.standard_normal((n, d))
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("standardize", [False, True])
def test_eigenface_pca_inverse_and_distance(synth, standardize):
    from eigenface import EigenfacePCA
    from eigenface.compat import sklearn_objects
    m = EigenfacePCA(8, standardize=standardize).fit(synth)
    scaler, pca = sklearn_objects(m)
    X = synth[:33]
    F = m.transform(X)
    got = m.inverse_transform(F)
    assert got.dtype == np.float64 and got.shape == X.shape
    np.testing.assert_array_equal(m.reconstruct(X), got)
    want = scaler.inverse_transform(pca.inverse_transform(F))
    # the bound, from the operands the engine holds (fp32 mean and R)
    from eigenface.pca import reconstruction_operands
    R, s = reconstruction_operands(m.components_, m.scaler_scale_ if standardize else None)
    tol = ru.recon_err(F, R, m._mu)
    # the fp32 storage of mean and R against sklearn's fp64 attributes: one rounding each
    tol = tol + ru.U32 * (np.abs(ru.f64(m._mu))[None, :] + ru.product_mag(F, R))
    err = np.abs(got - want)
    print(f"standardize={standardize}: max err/bound {np.max(err / tol):.3g}")
    assert np.all(err <= tol)
    # distance from face space against the same objects' fp64 residual (the scaler's space)
    z = scaler.transform(X.astype(np.float64))
    direct = ((z - pca.inverse_transform(pca.transform(z))) ** 2).sum(axis=1)
    e2 = m.face_distance(X)
    assert e2.dtype == np.float64 and e2.shape == (33,)
    # bound: the engine's path from its fp32 operands, end to end (projection error through |R|)
    c = ru.centred_ref(X, m._mu)
    F64 = c @ ru.f64(m._W)
    extra = (2e-6 * (np.abs(c) @ np.abs(ru.f64(m._W))) + 1e-6) @ np.abs(ru.f64(R))
    r = ru.residual_ref(X, F64, R, m._mu, s)
    bound = ru.sumsq_bound(r, ru.residual_err(X, F64, R, m._mu, s, extra), X.shape[1] + 8)
    # and the fp32 storage of the operands against the fp64 attributes
    # (one rounding each of mean, R, W and s: W's goes through the features and |R|)
    store = ru.U32 * (np.abs(ru.f64(m._mu))[None, :] + ru.product_mag(F64, R)
                      + (np.abs(c) @ np.abs(ru.f64(m._W))) @ np.abs(ru.f64(R)))
    store = (store if s is None else store * ru.f64(s)[None, :]) + ru.U32 * np.abs(r)
    bound = bound + (2.0 * np.abs(r) * store + store * store).sum(axis=1)
    assert np.all(np.abs(e2 - direct) <= bound), float(np.max(np.abs(e2 - direct) / bound))
    np.testing.assert_allclose(m.face_distance(X, squared=False), np.sqrt(e2))
    # faces the model was fitted on lie nearer to face space than noise does
    noise = np.random.default_rng(14).integers(0, 256, X.shape, dtype=np.uint8)
    assert np.median(m.face_distance(noise)) > 4 * np.median(e2)


def test_compat_layouts(synth):
    import eigenface
    from eigenface import EigenfacePCA, manual_pca
    from eigenface.compat import sklearn_objects
    X = synth[:21]
    # face_model.pkl layout: real sklearn objects, populated as compat writes them
    m = EigenfacePCA(8, standardize=True).fit(synth)
    scaler, pca = sklearn_objects(m)
    md = {"pca": pca, "scaler": scaler}
    z = scaler.transform(X.astype(np.float64))
    f = pca.transform(z)
    want = scaler.inverse_transform(pca.inverse_transform(f))
    got = eigenface.reconstruct_faces(X, md, dtype="float32")
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-3)  # fp32 projection and product of 8-bit pixels
    u8 = eigenface.reconstruct_faces(X, md)
    assert u8.dtype == np.uint8 and np.abs(u8.astype(np.int32) - np.rint(np.clip(want, 0, 255))).max() <= 1
    e2 = eigenface.face_space_distance(X, md)
    direct = ((z - pca.inverse_transform(f)) ** 2).sum(axis=1)
    np.testing.assert_allclose(e2, direct, rtol=1e-4)
    # models/*_pca_model.pkl layout
    ef, mean_face, proj, lam = manual_pca(synth, 8)
    md2 = {"eigenfaces": ef, "mean_face": mean_face}
    f2 = (X - mean_face) @ ef
    want2 = mean_face + f2 @ ef.T
    np.testing.assert_allclose(eigenface.reconstruct_faces(X, md2, dtype="float32"), want2, rtol=0, atol=2e-3)
    np.testing.assert_allclose(eigenface.face_space_distance(X, md2), ((X - want2) ** 2).sum(axis=1), rtol=1e-4)
    # one face, as the recognise drop-ins take it
    assert eigenface.face_space_distance(X[0], md2).shape == (1,)
    # back to the first dict: its model and its way back are uploaded again
    np.testing.assert_allclose(eigenface.face_space_distance(X, md), direct, rtol=1e-4)
