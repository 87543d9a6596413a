"""Model bank: distance from face space per slot and the face gate on the GPU (ef_bank_recon_set,
ef_bank_face_distance, ef_bank_recognize_gated) against the fp64 reference and the bounds of
tests/recon_util.py.

As in tests/test_gpu_recon.py the residual's reference is evaluated at the features the call
returned, with residual_err and sumsq_bound at terms = d + k: the grouped kernel runs the same
tile walk per (slot, probe tile, pixel split) and a fixed-order sum over the splits, so the
single-model bounds hold per (probe, slot).
"""
import numpy as np
import pytest

import recon_util as ru

pytestmark = pytest.mark.gpu

EF_E_INVALID, EF_E_STATE = -1, -3

_models = {}


def _model(d, k, weighted, tag=0, s_lo=0.02):
    """(mean, W (d, k), R (k, d), s or None) as fp32, as tests/test_gpu_recon.py::_model builds
    them: orthonormal rows V, and with a weight s ~ U(0.02, 1) the standardised form
    W = diag(s) V^T, R = V diag(1/s).  tag tells models of one shape apart; s_lo narrows the weights."""
    key = (d, k, weighted, tag, s_lo)
    if key not in _models:
        rng = np.random.default_rng(1000 * d + 10 * k + weighted + 7919 * tag)
        V = ru.orthonormal_rows(rng, k, d)
        mean = rng.uniform(100.0, 156.0, d).astype(np.float32)
        if weighted:
            s = rng.uniform(s_lo, 1.0, d)
            W, R, s = ru.standardised_operands(V, 1.0 / s)
            s = s.astype(np.float32)
        else:
            W, R, s = V.T, V, None
        _models[key] = (mean, np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(R, dtype=np.float32), s)
    return _models[key]


def _near(rng, b, mean, R, s):
    """Pixels near a model's face space (tests/test_gpu_recon.py::_pixels, kind "near")."""
    d, k = mean.shape[0], R.shape[0]
    amp = 15.0 * np.sqrt(d / k) * (1.0 if s is None else float(s.min()))
    f0 = rng.standard_normal((b, k)) * amp
    return np.clip(np.rint(ru.reconstruct_ref(f0, R, mean)), 0, 255).astype(np.uint8)


def _fill(eng, models, recon=True, gallery_rows=2):
    eng.bank_clear()
    for m, (mean, W, R, s) in enumerate(models):
        g = np.random.default_rng(m).standard_normal((gallery_rows, W.shape[1])).astype(np.float32)
        assert eng.bank_add(mean, W, g) == m
        if recon:
            eng.bank_set_reconstruction(m, R, s)


def _check_slot(P, model, F, eps2, energy, what):
    """One slot's column of the results against fp64 at the returned features F (b, k)."""
    mean, W, R, s = model
    d, k = mean.shape[0], R.shape[0]
    r = ru.residual_ref(P, F, R, mean, s)
    e = ru.residual_err(P, F, R, mean, s)
    ref = (r * r).sum(axis=1)
    bound = ru.sumsq_bound(r, e, d + k)
    err = np.abs(ru.f64(eps2) - ref)
    c = ru.centred_ref(P, mean, s)
    ec = ru.residual_err(P, np.zeros_like(ru.f64(F)), R, mean, s)
    eref = (c * c).sum(axis=1)
    eb = ru.sumsq_bound(c, ec, d + k)
    eerr = np.abs(ru.f64(energy) - eref)
    print(f"{what}: eps2 / E {np.median(ref / eref):.3g}  eps2 err/bound {np.max(err / bound):.3g}  "
          f"E err/bound {np.max(eerr / eb):.3g}")
    assert np.all(err <= bound), (what, float(np.max(err / bound)))
    assert np.all(eerr <= eb), (what, float(np.max(eerr / eb)))


def _check_bank(eng, P, models, what):
    b, M = P.shape[0], len(models)
    eps2, energy, feats = eng.bank_face_distance(P, return_energy=True, return_features=True)
    assert eps2.shape == (b, M) and energy.shape == (b, M) and eps2.dtype == np.float32
    assert [f.shape for f in feats] == [(b, m[1].shape[1]) for m in models]
    for m, model in enumerate(models):
        _check_slot(P, model, feats[m], eps2[:, m], energy[:, m], f"{what} slot {m}")
    return eps2, energy, feats


MIXED_D = 4096
MIXED_KS = (5, 20, 50, 100, 601)  # kp 16, 32, 64, 128, 640


def _mixed(ks):
    return [_model(MIXED_D, k, MIXED_KS.index(k) % 2 == 1) for k in ks]


def _mixed_pixels(kind, b, models):
    rng = np.random.default_rng(b + len(models))
    if kind == "random":
        return rng.integers(0, 256, (b, MIXED_D), dtype=np.uint8)
    # row i lies near the face space of slot 0, 2, 4, ... in turn
    P = np.empty((b, MIXED_D), np.uint8)
    targets = list(range(0, len(models), 2))
    for i, t in enumerate(targets):
        rows = np.arange(i, b, len(targets))
        mean, W, R, s = models[t]
        P[rows] = _near(rng, len(rows), mean, R, s)
    return P


@pytest.mark.parametrize("b", [1, 129, 300])
@pytest.mark.parametrize("ks", [MIXED_KS, MIXED_KS[1:]], ids=["rk16", "rk32"])
def test_mixed_bank_against_fp64(eng, ks, b):
    """k = 5 pads to 16 components, which makes the whole launch use 16-component stages; the bank
    of the wider slots alone uses 32."""
    models = _mixed(ks)
    _fill(eng, models)
    for kind in ("random", "near"):
        P = _mixed_pixels(kind, b, models)
        _check_bank(eng, P, models, f"{len(ks)} slots b={b} {kind}")


@pytest.mark.parametrize("d", [333, 200])
def test_ragged_d(eng, d):
    """d = 333: no vector loads, R padded to 384 columns; d = 200: vector loads, one partial tile."""
    models = [_model(d, k, i % 2 == 1) for i, k in enumerate((1, 10, 33))]
    _fill(eng, models)
    rng = np.random.default_rng(d)
    _check_bank(eng, rng.integers(0, 256, (3, d), dtype=np.uint8), models, f"d={d} random")
    P = np.concatenate([_near(rng, 1, m[0], m[2], m[3]) for m in models])
    _check_bank(eng, P, models, f"d={d} near")


def test_both_split_regimes_and_slot_independence(eng):
    from eigenface import bank_recon_schedule
    # one pixel split: 600 slots of k = 4 at d = 256, one probe
    d, M = 256, 600
    assert bank_recon_schedule(1, d, M)["nsplit"] == 1
    models = [_model(d, 4, m % 2 == 1, tag=m) for m in range(M)]
    _fill(eng, models, gallery_rows=1)
    rng = np.random.default_rng(3)
    P = rng.integers(0, 256, (1, d), dtype=np.uint8)
    eps2, energy, feats = eng.bank_face_distance(P, return_energy=True, return_features=True)
    worst = 0.0
    for m, (mean, W, R, s) in enumerate(models):
        r = ru.residual_ref(P, feats[m], R, mean, s)
        bound = ru.sumsq_bound(r, ru.residual_err(P, feats[m], R, mean, s), d + 4)
        err = np.abs(ru.f64(eps2[:, m]) - (r * r).sum(axis=1))
        c = ru.centred_ref(P, mean, s)
        eb = ru.sumsq_bound(c, ru.residual_err(P, np.zeros((1, 4)), R, mean, s), d + 4)
        eerr = np.abs(ru.f64(energy[:, m]) - (c * c).sum(axis=1))
        assert np.all(err <= bound) and np.all(eerr <= eb), m
        worst = max(worst, float(np.max(err / bound)), float(np.max(eerr / eb)))
    print(f"600 slots, nsplit 1: max err/bound {worst:.3g}")
    # slot 77 alone: the same reference, the same bounds
    _fill(eng, [models[77]])
    _check_bank(eng, P, [models[77]], "slot 77 alone")

    # many pixel splits: d = 4096 with two slots
    d = 4096
    assert bank_recon_schedule(1, d, 2)["nsplit"] > 1
    x, y = _model(d, 50, True), _model(d, 100, False)
    others = [_model(d, k, i % 2 == 0, tag=50 + i) for i, k in enumerate((20, 50, 7, 100, 33))]
    P = np.concatenate([rng.integers(0, 256, (2, d), dtype=np.uint8), _near(rng, 2, x[0], x[2], x[3])])
    for bank, at, what in (([x, y], 0, "first of two"), ([x], 0, "alone"), (others + [x], 5, "behind five others")):
        assert bank_recon_schedule(len(P), d, len(bank))["nsplit"] > 1
        _fill(eng, bank)
        eps2, energy, feats = eng.bank_face_distance(P, return_energy=True, return_features=True)
        _check_slot(P, x, feats[at], eps2[:, at], energy[:, at], f"nsplit > 1, {what}")


def test_f32_pixels_and_device_tensors(eng):
    import torch
    models = _mixed(MIXED_KS[1:4])
    _fill(eng, models)
    rng = np.random.default_rng(17)
    b = 129
    P32 = rng.uniform(0, 255, (b, MIXED_D)).astype(np.float32)
    h32 = _check_bank(eng, P32, models, "f32 pixels")
    P8 = rng.integers(0, 256, (b, MIXED_D), dtype=np.uint8)
    h8 = eng.bank_face_distance(P8, return_energy=True, return_features=True)
    dev = torch.device("cuda", eng.device)
    for P, host in ((P32, h32), (P8, h8)):
        t_eps, t_en, t_f = eng.bank_face_distance(torch.from_numpy(P).to(dev), return_energy=True, return_features=True)
        eng.synchronize()
        np.testing.assert_array_equal(t_eps.cpu().numpy(), host[0])
        np.testing.assert_array_equal(t_en.cpu().numpy(), host[1])
        np.testing.assert_array_equal(t_f.cpu().numpy(), np.concatenate(host[2], axis=1))
    # without the optional outputs: the same distances
    np.testing.assert_array_equal(eng.bank_face_distance(P8), h8[0])
    t = eng.bank_face_distance(torch.from_numpy(P8).to(dev))
    eng.synchronize()
    np.testing.assert_array_equal(t.cpu().numpy(), h8[0])
    # device operands of bank_set_reconstruction give the same state
    mean, W, R, s = models[0]
    eng.bank_set_reconstruction(0, torch.from_numpy(R).to(dev), torch.from_numpy(s).to(dev))
    np.testing.assert_array_equal(eng.bank_face_distance(P8), h8[0])


def test_deterministic_and_features_are_the_bank_s(eng):
    models = _mixed(MIXED_KS)
    _fill(eng, models)
    P = np.random.default_rng(18).integers(0, 256, (300, MIXED_D), dtype=np.uint8)
    a = eng.bank_face_distance(P, return_energy=True, return_features=True)
    c = eng.bank_face_distance(P, return_energy=True, return_features=True)
    np.testing.assert_array_equal(a[0], c[0])
    np.testing.assert_array_equal(a[1], c[1])
    feats = eng.bank_recognize(P, "cosine", return_features=True)[3]
    for fa, fc, fr in zip(a[2], c[2], feats):
        np.testing.assert_array_equal(fa, fc)
        np.testing.assert_array_equal(fa, fr)
    assert np.all(a[0] > 0)
    # four launches whatever M is: the two timed ones run once each per call
    eng.timing_reset()
    eng.timing(True)
    try:
        eng.bank_face_distance(P)
        (ms, n), (ms2, n2) = eng.timing_get("recon"), eng.timing_get("recon_reduce")
        assert n == 1 and n2 == 1 and ms > 0 and ms2 > 0
        assert eng.timing_get("project")[1] == 1 and eng.timing_get("search")[1] == 0
    finally:
        eng.timing(False)
        eng.timing_reset()


GATE_D, GATE_K, GATE_N = 4096, 50, 40


def _gate_case():
    """Four models of k = 50 with galleries of 40 rows, and 12 probes: row i < 4 planted in model
    i's face space (it is the source of that model's gallery row 3 i), four rows of uniform
    noise, four zero rows.  The margins are asserted on the fp64 reference, before any GPU call."""
    # (weights of U(0.5, 1): with the 0.02 of the other tests a planted row's pixel rounding alone is
    # a quarter of its weighted energy, which leaves no margin to plant anything)
    models = [_model(GATE_D, GATE_K, m % 2 == 1, tag=100 + m, s_lo=0.5) for m in range(4)]
    rng = np.random.default_rng(19)
    sources = [_near(rng, GATE_N, mean, R, s) for mean, W, R, s in models]
    galleries = [(ru.centred_ref(src, mean) @ ru.f64(W)).astype(np.float32)
                 for src, (mean, W, R, s) in zip(sources, models)]
    P = np.concatenate([np.stack([sources[m][3 * m] for m in range(4)]),
                        rng.integers(0, 256, (4, GATE_D), dtype=np.uint8), np.zeros((4, GATE_D), np.uint8)])
    ratio = np.empty((12, 4))
    eps_ref = np.empty((12, 4))
    for m, (mean, W, R, s) in enumerate(models):
        F = ru.centred_ref(P, mean) @ ru.f64(W)
        r = ru.residual_ref(P, F, R, mean, s)
        c = ru.centred_ref(P, mean, s)
        eps_ref[:, m] = (r * r).sum(axis=1)
        ratio[:, m] = eps_ref[:, m] / (c * c).sum(axis=1)
    own = ratio[np.arange(4), np.arange(4)]
    print(f"planted eps2/E max {own.max():.3g}, noise min {ratio[4:8].min():.3g}, zero rows min {ratio[8:].min():.3g}")
    assert np.all(own < 0.025), own
    assert np.all(ratio[4:8] > 0.4), ratio[4:8].min()
    return {"models": models, "galleries": galleries, "P": P, "ratio": ratio, "eps_ref": eps_ref}


@pytest.fixture(scope="module")
def gate_case():
    return _gate_case()


def _fill_gate_case(eng, case):
    eng.bank_clear()
    for (mean, W, R, s), g in zip(case["models"], case["galleries"]):
        eng.bank_set_reconstruction(eng.bank_add(mean, W, g), R, s)


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_gated_recognise(eng, gate_case, metric):
    from eigenface import best_over_models, decode_keys, face_gate_mask
    P, M = gate_case["P"], 4
    _fill_gate_case(eng, gate_case)
    keys0, rec0, best0, feats0 = eng.bank_recognize_raw(P, metric, matches=True, features=True)
    eps0, en0 = eng.bank_face_distance(P, return_energy=True)
    # an absolute gate per model a factor 4 above its planted row and far below everything else
    abs_gate = (4.0 * gate_case["eps_ref"][np.arange(4), np.arange(4)]).astype(np.float32)
    others = gate_case["eps_ref"].copy()
    others[np.arange(4), np.arange(4)] = np.inf
    assert np.all(others.min(axis=0) > 4.0 * abs_gate)
    inf = np.full(M, np.inf, np.float32)
    for gate, relative in ((np.full(M, 0.1, np.float32), True), (abs_gate, False), (inf, True), (inf, False),
                           (np.full(M, np.nan, np.float32), True)):
        keys, rec, best, feats, eps2, energy = eng.bank_recognize_gated_raw(P, gate, metric, relative=relative,
                                                                           matches=True, features=True)
        np.testing.assert_array_equal(keys, keys0)
        np.testing.assert_array_equal(rec.view(np.uint8), rec0.view(np.uint8))
        np.testing.assert_array_equal(feats, feats0)
        np.testing.assert_array_equal(eps2, eps0)
        np.testing.assert_array_equal(energy, en0)
        _, score = decode_keys(keys.reshape(-1), metric)
        mask = face_gate_mask(eps2, energy, gate, relative)
        np.testing.assert_array_equal(best, best_over_models(score.reshape(keys.shape), metric, allowed=mask))
        if not np.all(np.isfinite(gate)):
            np.testing.assert_array_equal(best, best0)  # +inf and NaN gate nothing
        else:
            assert best[:4].tolist() == [0, 1, 2, 3], best   # planted rows: their own slot
            assert best[4:8].tolist() == [-1] * 4, best       # noise: nobody
            assert mask[np.arange(4), np.arange(4)].all() and not mask[4:8].any()
    # the high-level form returns the same, and without the optional outputs nothing else changes
    idx, score, best, eps2, energy = eng.bank_recognize_gated(P, np.full(M, 0.1, np.float32), metric)
    np.testing.assert_array_equal(eps2, eps0)
    assert best[:8].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    # device tensors, the gate on the device too
    import torch
    dev = torch.device("cuda", eng.device)
    out = eng.bank_recognize_gated_raw(torch.from_numpy(P).to(dev), torch.full((M,), 0.1, device=dev), metric,
                                       matches=True, features=True)
    eng.synchronize()
    np.testing.assert_array_equal(out[0].cpu().numpy(), keys0)
    np.testing.assert_array_equal(out[2].cpu().numpy(), best)
    np.testing.assert_array_equal(out[3].cpu().numpy(), feats0)
    np.testing.assert_array_equal(out[4].cpu().numpy(), eps0)
    np.testing.assert_array_equal(out[5].cpu().numpy(), en0)


def test_state_rules():
    from eigenface import EigenfaceError, Engine
    d = 333
    models = [_model(d, k, i % 2 == 1) for i, k in enumerate((1, 10, 33))]
    cm = _model(d, 10, True)
    P = np.random.default_rng(20).integers(0, 256, (5, d), dtype=np.uint8)
    gate = np.full(3, 0.1, np.float32)

    def raises(code, call, text=None):
        with pytest.raises(EigenfaceError) as ei:
            call()
        assert ei.value.code == code, ei.value
        if text:
            assert text in str(ei.value), ei.value

    with Engine(0) as e:
        # the context's own model, gallery and reconstruction state
        e.set_model(cm[0], cm[1])
        e.set_reconstruction(cm[2], cm[3])
        e.set_gallery(np.random.default_rng(1).standard_normal((9, 10)).astype(np.float32))
        before = e.face_distance(P, return_energy=True, return_features=True)
        keys_before = e.recognize_keys(P, "l2")
        raises(EF_E_STATE, lambda: e.bank_face_distance(P))  # an empty bank
        _fill(e, models, recon=False)
        raises(EF_E_STATE, lambda: e.bank_face_distance(P), "slot 0")
        e.bank_set_reconstruction(0, models[0][2], models[0][3])
        e.bank_set_reconstruction(2, models[2][2], models[2][3])
        raises(EF_E_STATE, lambda: e.bank_face_distance(P), "slot 1")
        raises(EF_E_STATE, lambda: e.bank_recognize_gated(P, gate), "slot 1")
        for slot in (-1, 3, 4096):
            raises(EF_E_INVALID, lambda: e.bank_set_reconstruction(slot, models[0][2], models[0][3]))
        e.bank_recognize(P)  # the ungated call needs none of it
        e.bank_set_reconstruction(1, models[1][2], models[1][3])
        want = e.bank_face_distance(P, return_energy=True)
        # a failed call leaves the slot's state: R of another d never reaches the library's copy
        with pytest.raises(ValueError):
            e.bank_set_reconstruction(1, models[1][2][:, :-1])
        np.testing.assert_array_equal(e.bank_face_distance(P), want[0])
        # replacing a slot's state: the same operands give the same bits, others give others
        e.bank_set_reconstruction(1, models[1][2], None)
        assert not np.array_equal(e.bank_face_distance(P)[:, 1], want[0][:, 1])
        e.bank_set_reconstruction(1, models[1][2], models[1][3])
        np.testing.assert_array_equal(e.bank_face_distance(P), want[0])
        # a later add keeps the earlier slots' state and is reported as lacking its own
        extra = _model(d, 20, False)
        assert e.bank_add(extra[0], extra[1], np.zeros((0, 20), np.float32)) == 3
        raises(EF_E_STATE, lambda: e.bank_face_distance(P), "slot 3")
        e.bank_set_reconstruction(3, extra[2], extra[3])
        got = e.bank_face_distance(P, return_energy=True)
        np.testing.assert_array_equal(got[0][:, :3], want[0])
        np.testing.assert_array_equal(got[1][:, :3], want[1])
        # b = 0: empty results, no error
        z = e.bank_face_distance(P[:0], return_energy=True, return_features=True)
        assert z[0].shape == (0, 4) and z[1].shape == (0, 4)
        assert [f.shape for f in z[2]] == [(0, 1), (0, 10), (0, 33), (0, 20)]
        zg = e.bank_recognize_gated(P[:0], np.full(4, 0.1, np.float32))
        assert zg[0].shape == (0, 4) and zg[3].shape == (0, 4)
        with pytest.raises(ValueError):
            e.bank_recognize_gated(P, gate)  # three bounds for four slots
        # the context's own state is untouched
        after = e.face_distance(P, return_energy=True, return_features=True)
        for a, c in zip(before, after):
            np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(e.recognize_keys(P, "l2"), keys_before)
        # clear drops everything
        e.bank_clear()
        raises(EF_E_STATE, lambda: e.bank_face_distance(P))
        _fill(e, models[:1], recon=False)
        raises(EF_E_STATE, lambda: e.bank_face_distance(P), "slot 0")
        after = e.face_distance(P, return_energy=True, return_features=True)
        for a, c in zip(before, after):
            np.testing.assert_array_equal(a, c)


def _person(seed, n=60, d=1024, rank=12):
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((rank, d))
    x = 128.0 + 6.0 * rng.standard_normal((n, rank)) @ basis + 1.5 * rng.standard_normal((n, d))
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def _e2e_bound(X, mu, W, R, s, k):
    """|eps2 - fp64 pipeline| of one engine path from its fp32 operands, the projection's error
    carried through |R| (tests/test_gpu_recon.py::test_end_to_end_fp64_pipeline)."""
    c = ru.centred_ref(X, mu)
    F64 = c @ ru.f64(W)
    extra = (2e-6 * (np.abs(c) @ np.abs(ru.f64(W))) + 1e-6) @ np.abs(ru.f64(R))
    r = ru.residual_ref(X, F64, R, mu, s)
    return (r * r).sum(axis=1), ru.sumsq_bound(r, ru.residual_err(X, F64, R, mu, s, extra), X.shape[1] + k)


def test_python_layer():
    import eigenface
    from eigenface import EigenfacePCA, ModelBank, get_engine, manual_pca
    from eigenface.bank import _operands
    from eigenface.compat import sklearn_objects
    from eigenface.pca import reconstruction_operands
    k = 12
    xa, xb = _person(31), _person(32)
    # face_model.pkl layout: real sklearn objects, populated as compat writes them
    m = EigenfacePCA(k, standardize=True).fit(xa)
    scaler, pca = sklearn_objects(m)
    ma = {"pca": pca, "scaler": scaler, "face_features": pca.transform(scaler.transform(xa.astype(np.float64))),
          "face_labels": [7] * len(xa), "person_id_map": {"alice": 7}}
    # models/*_pca_model.pkl layout, with the gallery keys the bank reads
    ef, mean_face, proj, lam = manual_pca(xb, k)
    mb = {"eigenfaces": ef, "mean_face": mean_face, "face_features": proj, "face_labels": [9] * len(xb),
          "person_id_map": {"bob": 9}}
    models = {"alice": {"model_data": ma}, "nobody": {"model_data": None}, "bob": {"model_data": mb}}
    rng = np.random.default_rng(33)
    noise = rng.integers(0, 256, (3, xa.shape[1]), dtype=np.uint8)
    rows = np.concatenate([xa[[5, 17]], xb[[7, 30]], noise])
    # the margins of the decision on the fp64 reference: faces a factor 4 inside the gate, noise outside
    ops = []
    for md in (ma, mb):
        mu, w, comps, scale = _operands(md)
        R, s = reconstruction_operands(comps, scale)
        ops.append((mu, w, R, s))
    ref = [_e2e_bound(rows, mu, w, R, s, k) for mu, w, R, s in ops]
    ratio = np.stack([e2 / (ru.centred_ref(rows, mu, s) ** 2).sum(axis=1)
                      for (e2, _), (mu, w, R, s) in zip(ref, ops)], axis=1)
    print("eps2 / E per (row, model):\n", np.array2string(ratio, precision=3))
    assert np.all(ratio[[0, 1], 0] < 0.025) and np.all(ratio[[2, 3], 1] < 0.025) and np.all(ratio[4:] > 0.4)

    plain = ModelBank(models)
    assert plain.names == ["alice", "bob"] and plain.gate is None
    # no gate: no R is uploaded, and the labels are the rule on the ungated call's results
    eng = get_engine(0)
    with pytest.raises(eigenface.EigenfaceError) as ei:
        eng.bank_face_distance(rows)
    assert ei.value.code == EF_E_STATE
    ungated = plain.recognize_rows(rows)
    idx, sim, _ = eng.bank_recognize(rows, "cosine")
    assert ungated == plain.label(idx, sim, 0.8)
    assert [u[:2] for u in ungated[:4]] == [(7, "alice"), (7, "alice"), (9, "bob"), (9, "bob")]
    with pytest.raises(ValueError):
        plain.is_face(rows)
    # face_distance uploads the ways back on first use, and agrees with the per-model path within the
    # two calls' bounds: each lies within its own bound of the fp64 pipeline
    eps2, energy = plain.face_distance(rows)
    assert eps2.dtype == np.float64 and eps2.shape == (7, 2) and energy.shape == (7, 2)
    for j, md in enumerate((ma, mb)):
        single = eigenface.face_space_distance(rows, md)
        e2, bound = ref[j]
        assert np.all(np.abs(eps2[:, j] - e2) <= bound) and np.all(np.abs(single - e2) <= bound)
        assert np.all(np.abs(eps2[:, j] - single) <= 2 * bound)
    assert plain.recognize_rows(rows) == ungated

    gated = ModelBank(models, face_gate=0.1)
    got = gated.recognize_rows(rows)
    assert got[:4] == ungated[:4]
    assert got[4:] == [(-1, "unknown", 0.0)] * 3
    assert gated.is_face(rows).tolist() == [True] * 4 + [False] * 3
    np.testing.assert_array_equal(gated.face_distance(rows)[0], eps2)
    # a dict gate: a missing name means no gate for that model
    half = ModelBank(models, face_gate={"alice": 0.1})
    assert half.gate.tolist() == [np.float32(0.1), np.inf] and half.gated.tolist() == [True, False]
    assert half.is_face(rows).tolist() == [True, True, False, False, False, False, False]
    lab = half.recognize_rows(rows)
    assert lab[:4] == ungated[:4]
    idx, sim, _ = get_engine(0).bank_recognize(rows, "cosine")
    allowed = np.ones((7, 2), bool)
    allowed[2:, 0] = False  # alice's gate rejects everything but her own two rows
    assert lab == half.label(idx, sim, 0.8, allowed=allowed)
    # the plain bank takes the engine back and behaves as before
    assert plain.recognize_rows(rows) == ungated
