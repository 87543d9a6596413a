"""Model bank on the GPU (ef_bank_*): grouped projection, grouped exact search, best-over-models.

The search is checked against unchanged project code (a second plain Engine's search_matches /
search_keys on the same features) and the fp64 checker of parity_util, never against the bank
itself.  An "identity model" (float32 pixels, zero mean, W = I) makes the bank's features equal
the pixels exactly (one non-zero product per sum), so a test can choose the features it wants.
"""
import numpy as np
import pytest

import parity_util
from conftest import golden
from oracle import eigenface_oracle as orc

pytestmark = pytest.mark.gpu

KS = [3, 16, 65, 128, 130, 520]   # kp 16, 16, 128, 128, 256 (two column tiles), 640 (run-time row length)
NS = [7, 1, 300, 0, 40, 600]
EF_KEY_NONE = (1 << 63) - 1
FORMS = {"u8_d4096": (4096, np.uint8), "u8_d100": (100, np.uint8), "f32_d4096": (4096, np.float32)}


def _models(form):
    """(means, Ws, galleries, 129 probe pixel rows) of one pixel form, built once."""
    d, dt = FORMS[form]
    rng = np.random.default_rng(100 + d + (dt == np.uint8))
    if dt == np.uint8:
        pix = rng.integers(0, 256, (129, d), dtype=np.uint8)
        mus = [rng.uniform(60, 200, d).astype(np.float32) for _ in KS]
    else:
        pix = rng.uniform(0, 1, (129, d)).astype(np.float32)
        mus = [rng.uniform(0, 1, d).astype(np.float32) for _ in KS]
    ws = [(rng.standard_normal((d, k)) / np.sqrt(d)).astype(np.float32) for k in KS]
    gs = []
    for mu, w, n in zip(mus, ws, NS):
        src = rng.integers(0, 256, (n, d)).astype(dt) if dt == np.uint8 else rng.uniform(0, 1, (n, d)).astype(dt)
        gs.append(orc.project(src, mu, w).astype(np.float32).reshape(n, w.shape[1]))
    return mus, ws, gs, pix


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(form):
        if form not in cache:
            cache[form] = _models(form)
        return cache[form]
    return get


@pytest.fixture(scope="module")
def plain():
    """A second, plain engine: the unchanged single-gallery search the bank is checked against."""
    from eigenface import Engine
    e = Engine(0)
    yield e
    e.close()


def _fill(eng, mus, ws, gs):
    eng.bank_clear()
    for i, (mu, w, g) in enumerate(zip(mus, ws, gs)):
        assert eng.bank_add(mu, w, g) == i


def _identity_bank(eng, galleries, d):
    """Slots whose features are the float32 pixels' first k columns exactly."""
    eng.bank_clear()
    for g in galleries:
        k = g.shape[1]
        eng.bank_add(np.zeros(d, np.float32), np.eye(d, k, dtype=np.float32), g)


@pytest.mark.parametrize("b", [1, 5, 129])
@pytest.mark.parametrize("form", list(FORMS))
def test_features_within_the_projection_bound_and_deterministic(eng, models, form, b):
    mus, ws, gs, pix = models(form)
    _fill(eng, mus, ws, gs)
    assert eng.bank_info() == (len(KS), FORMS[form][0], sum(KS), sum(NS))
    p = pix[:b]
    keys, _, best, feats = eng.bank_recognize_raw(p, "cosine", features=True)
    assert keys.shape == (b, len(KS)) and feats.shape == (b, sum(KS)) and best.shape == (b,)
    off = 0
    for mu, w in zip(mus, ws):
        k = w.shape[1]
        ref = orc.project(p, mu.astype(np.float64), w.astype(np.float64))
        bound = np.abs(p.astype(np.float64) - mu) @ np.abs(w.astype(np.float64))
        err = np.abs(feats[:, off:off + k] - ref)
        print(f"{form} b={b} k={k}: max err/bound {np.max(err / (2e-6 * bound + 1e-6)):.3f}")
        assert np.all(err <= 2e-6 * bound + 1e-6)  # the bound tests/test_gpu_project.py holds ef_project to
        off += k
    keys2, _, best2, feats2 = eng.bank_recognize_raw(p, "cosine", features=True)
    np.testing.assert_array_equal(feats.view(np.int32), feats2.view(np.int32))
    np.testing.assert_array_equal(keys, keys2)
    np.testing.assert_array_equal(best, best2)
    # the high-level form: per-slot feature arrays, decoded scores
    idx, score, best3, fl = eng.bank_recognize(p, "cosine", return_features=True)
    assert [f.shape for f in fl] == [(b, k) for k in KS]
    np.testing.assert_array_equal(np.concatenate(fl, axis=1), feats)
    np.testing.assert_array_equal(best3, best)
    assert (idx[:, 3] == -1).all() and np.isnan(score[:, 3]).all() and (keys[:, 3] == EF_KEY_NONE).all()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_search_equals_the_plain_engine_bit_for_bit(eng, plain, models, metric):
    mus, ws, gs, pix = models("u8_d4096")
    _fill(eng, mus, ws, gs)
    keys, rec, best, feats = eng.bank_recognize_raw(pix, metric, matches=True, features=True)
    from eigenface import decode_keys
    off = 0
    for m, (g, k) in enumerate(zip(gs, KS)):
        f = np.ascontiguousarray(feats[:, off:off + k])
        off += k
        np.testing.assert_array_equal(rec["key"][:, m], keys[:, m])
        if len(g) == 0:
            assert (keys[:, m] == EF_KEY_NONE).all() and np.isinf(rec["score"][:, m]).all()
            assert (rec["scale"][:, m] == 0).all()
            continue
        plain.set_gallery(g)
        want = plain.search_matches(f, metric)
        np.testing.assert_array_equal(rec["key"][:, m], want["key"])
        np.testing.assert_array_equal(rec["score"][:, m].view(np.int64), want["score"].view(np.int64))
        np.testing.assert_array_equal(rec["scale"][:, m].view(np.int64), want["scale"].view(np.int64))
        idx, _ = decode_keys(keys[:, m], metric)
        parity_util.assert_exact_argbest(f, g, idx, metric)


def test_ties_first_index(eng, plain):
    """tests/golden/ties.npz as one slot's gallery, plus a duplicate row, a row and its 2.5x
    multiple, a zero row and a zero probe: the same rows as search_keys, the lowest index of a tie."""
    t = golden("ties.npz")
    g = t["gallery"].astype(np.float32)
    q = t["probes"].astype(np.float32)
    g = np.concatenate([g, g[14:15], np.float32(2.5) * g[9:10], np.zeros((1, 8), np.float32)])
    q = np.concatenate([q, g[14:15], g[9:10], np.float32(2.5) * g[9:10], np.zeros((1, 8), np.float32)])
    _identity_bank(eng, [g], 8)
    idx, sim, best, feats = eng.bank_recognize(q, "cosine", return_features=True)
    np.testing.assert_array_equal(feats[0], q)  # the identity model: features are the pixels
    np.testing.assert_array_equal(idx[:6, 0], t["idx"])
    np.testing.assert_allclose(sim[:6, 0], t["sim"], atol=1e-6)
    # np.argmax on rounded unit rows cannot order a row and its multiple: the tie-window checker
    parity_util.assert_exact_argbest(q, g, idx[:, 0], "cosine")
    assert idx[6, 0] == 14 and idx[7, 0] == 9 and idx[8, 0] == 9 and idx[9, 0] == 0 and sim[9, 0] == 0
    plain.set_gallery(g)
    for metric in ("cosine", "l2"):
        keys = eng.bank_recognize_raw(q, metric)[0]
        np.testing.assert_array_equal(keys[:, 0], plain.search_keys(q, metric))
    assert best[9] == -1  # a zero probe has similarity 0 everywhere: no model wins


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_row_slices_do_not_change_the_answer(eng, plain, metric):
    """n = 5000 rows at k = 16: twenty row slices.  Duplicates of the best row sit in the first
    and the last slice; the lowest index wins, alone or after five other slots."""
    rng = np.random.default_rng(21)
    g = rng.standard_normal((5000, 16)).astype(np.float32)
    q = rng.standard_normal((9, 16)).astype(np.float32)
    first = np.array([3, 255, 100, 17, 0, 200, 31, 64, 128])
    last = np.array([4999, 4864, 4900, 4990, 4870, 4999 - 7, 4888, 4950, 4865])
    g[first] = q
    g[last] = q
    g[2500:2505] = q[:5]  # and one in the middle
    others = [rng.standard_normal((n, k)).astype(np.float32) for n, k in [(7, 3), (300, 16), (0, 5), (600, 16), (40, 9)]]
    _identity_bank(eng, [g], 16)
    alone = eng.bank_recognize_raw(q, metric, matches=True)
    _identity_bank(eng, others + [g], 16)
    after = eng.bank_recognize_raw(q, metric, matches=True)
    from eigenface import decode_keys
    idx, _ = decode_keys(alone[0][:, 0], metric)
    np.testing.assert_array_equal(idx, first)
    np.testing.assert_array_equal(alone[0][:, 0], after[0][:, 5])
    for f in ("score", "scale", "key"):
        np.testing.assert_array_equal(alone[1][f][:, 0].view(np.int64), after[1][f][:, 5].view(np.int64))
    plain.set_gallery(g)
    want = plain.search_matches(q, metric)
    for f in ("score", "scale", "key"):
        np.testing.assert_array_equal(alone[1][f][:, 0].view(np.int64), want[f].view(np.int64))


def test_best_slot(eng):
    from eigenface import best_over_models
    rng = np.random.default_rng(31)
    d = 16
    q = rng.standard_normal((12, d)).astype(np.float32)
    ga = rng.standard_normal((50, d)).astype(np.float32)
    gb = rng.standard_normal((70, d)).astype(np.float32)
    # the same model twice: the lower slot keeps it (a later equal score is not strictly greater)
    _identity_bank(eng, [gb, ga, ga], d)
    for metric in ("cosine", "l2"):
        idx, score, best = eng.bank_recognize(q, metric)
        np.testing.assert_array_equal(score[:, 1], score[:, 2])
        assert not (best == 2).any()
        np.testing.assert_array_equal(best, best_over_models(score, metric))
    # one slot holds the probes' own projections
    own = np.concatenate([ga[:20], q])
    _identity_bank(eng, [ga, np.zeros((0, d), np.float32), own, gb], d)
    for metric in ("cosine", "l2"):
        idx, score, best = eng.bank_recognize(q, metric)
        np.testing.assert_array_equal(best, np.full(12, 2))
        np.testing.assert_array_equal(idx[:, 2], 20 + np.arange(12))
        np.testing.assert_array_equal(best, best_over_models(score, metric))
    # probes opposite (rows 0..5) or orthogonal (rows 6..11) to every gallery row: no similarity > 0
    gp = np.abs(ga)
    gp[:, 8:] = 0
    qn = -np.abs(q)
    qn[6:, :8] = 0
    qn[:6, 8:] = 0
    _identity_bank(eng, [gp, gp[:10] * np.float32(2)], d)
    idx, score, best = eng.bank_recognize(qn, "cosine")
    assert (score[:6] < 0).all() and (score[6:] == 0).all()
    np.testing.assert_array_equal(best, np.full(12, -1))
    np.testing.assert_array_equal(best, best_over_models(score, "cosine"))
    idx, score, best = eng.bank_recognize(qn, "l2")  # L2 always has a nearest model
    assert (best >= 0).all()
    np.testing.assert_array_equal(best, best_over_models(score, "l2"))


def test_state_errors_and_the_context_is_untouched(eng, models):
    import torch
    from eigenface import EigenfaceError
    mus, ws, gs, pix = models("u8_d4096")
    # the context's own model and gallery, before any bank use
    eng.set_model(mus[2], ws[2])
    eng.set_gallery(gs[2])
    before = eng.recognize_keys(pix, "l2")
    eng.bank_clear()
    assert eng.bank_info() == (0, 0, 0, 0)
    with pytest.raises(EigenfaceError, match="EF_E_STATE"):
        eng.bank_recognize(pix[:3])
    _fill(eng, mus, ws, gs)
    info = eng.bank_info()
    with pytest.raises(EigenfaceError, match="EF_E_INVALID"):
        eng.bank_add(np.zeros(100, np.float32), np.zeros((100, 4), np.float32), np.zeros((2, 4), np.float32))
    assert eng.bank_info() == info
    host = eng.bank_recognize_raw(pix, "cosine", matches=True, features=True)
    # device tensors: the same keys, records, choice and features, stream-ordered
    dev = eng.bank_recognize_raw(torch.as_tensor(pix, device="cuda"), "cosine", matches=True, features=True)
    np.testing.assert_array_equal(dev[0].cpu().numpy(), host[0])
    np.testing.assert_array_equal(dev[1].cpu().numpy().reshape(-1), host[1].view(np.int64).reshape(-1))
    np.testing.assert_array_equal(dev[2].cpu().numpy(), host[2])
    np.testing.assert_array_equal(dev[3].cpu().numpy().view(np.int32), host[3].view(np.int32))
    # slots added from device tensors hold the same data
    eng.bank_clear()
    for mu, w, g in zip(mus, ws, gs):
        eng.bank_add(*(torch.as_tensor(a, device="cuda") for a in (mu, w, g)))
    assert eng.bank_info() == info
    np.testing.assert_array_equal(eng.bank_recognize_raw(pix, "cosine")[0], host[0])
    assert eng.bank_recognize(pix[:0])[0].shape == (0, len(KS))  # b = 0
    # the context's single model and gallery answer as before, with the bank in place and after
    np.testing.assert_array_equal(eng.recognize_keys(pix, "l2"), before)
    eng.bank_clear()
    assert eng.bank_info() == (0, 0, 0, 0)
    np.testing.assert_array_equal(eng.recognize_keys(pix, "l2"), before)


def _trained(person, n, seed):
    from eigenface.compat import FaceTrainer
    x, _ = orc.synth_faces(n, 64, r=32, seed=seed)
    tr = FaceTrainer()
    tr.face_images = x
    tr.face_info = [{"face_id": i} for i in range(n)]
    tr.assign_labels_interactive(person)
    assert tr.train_pca_model()
    return x, tr.model_dict()


def test_model_bank_labels_like_recognize_faces_all_models(capsys):
    """Two FaceTrainer models, a None model and one with a broken scaler.  Names and ids are
    those of recognize_faces_all_models; confidences agree within the two projections' error
    bounds carried through the cosine:

    both paths compute fp32 features within e_j = 2e-6 (|p - mu| . |W|)_j + 1e-6 of the exact
    ones (the bound of tests/test_gpu_project.py), so they differ by a vector delta with
    ||delta|| <= 2 ||e||.  A unit vector moves by at most 2 ||delta|| / ||f|| when f moves by
    delta, so every row's cosine moves by at most 4 ||e|| / ||f||, and so does their maximum
    (the winning row may change; the maximum is 1-Lipschitz in the sup norm).  Each path rounds
    its fp64 cosine to fp32 once: 2 x 2^-24 more."""
    from eigenface import ModelBank
    from eigenface.compat import _folded, recognize_faces_all_models
    xa, ma = _trained("alice", 120, 1)
    xb, mb = _trained("bob", 90, 2)
    broken = dict(mb)
    broken["scaler"] = object()
    models = {"nobody": {"model_data": None}, "alice": {"model_data": ma}, "broken": {"model_data": broken},
              "bob": {"model_data": mb}}
    rng = np.random.default_rng(5)
    rows = np.concatenate([xa[[5, 17]], xb[[7, 30]],
                           np.clip(xa[[40]].astype(np.int32) + rng.integers(-6, 7, (1, 4096)), 0, 255).astype(np.uint8)])
    faces = [r.reshape(64, 64) for r in rows]
    capsys.readouterr()
    bank = ModelBank(models)
    out = capsys.readouterr().out
    assert "Error recognizing with model broken:" in out and "nobody" not in out
    assert bank.names == ["alice", "bob"] and len(bank) == 2
    got = bank.recognize_faces(faces, 0.8)
    want = recognize_faces_all_models(faces, models, 0.8)
    assert [g[:2] for g in got] == [w[:2] for w in want]
    assert [g[1] for g in got] == ["alice", "alice", "bob", "bob", "alice"]
    tol = np.zeros(len(rows))
    for md in (ma, mb):
        mu, w = _folded(md)
        e = 2e-6 * (np.abs(rows.astype(np.float64) - mu) @ np.abs(w.astype(np.float64))) + 1e-6
        f = orc.project(rows, mu, w)
        tol = np.maximum(tol, 4 * np.linalg.norm(e, axis=1) / np.linalg.norm(f, axis=1) + 2.0 ** -23)
    for g, w, t in zip(got, want, tol):
        print(f"confidence {g[2]:.9f} vs {w[2]:.9f}, bound {t:.3e}")
        assert abs(g[2] - w[2]) <= t
    # an in-place edit is picked up by refresh(); another bank on the same engine by itself
    models["bob"]["model_data"] = None
    assert bank.refresh().names == ["alice"]
    assert [g[1] for g in bank.recognize_faces(faces[:2], 0.8)] == ["alice", "alice"]
    assert ModelBank({}).recognize_faces(faces[:1]) == [(-1, "unknown", 0.0)]
    assert [g[1] for g in bank.recognize_faces(faces[:2], 0.8)] == ["alice", "alice"]
