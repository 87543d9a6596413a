"""Host side of the leave-one-out evaluation (eigenface/evaluate.py): open-set rates from
packed keys on a hand-written example, and the Python-side checks of the labelled search.
No GPU needed."""
import ctypes

import numpy as np
import pytest


def _keys(pairs, metric):
    """pairs: (score, row) or None per probe -> packed keys (cosine keys hold -similarity)."""
    from eigenface import _native as N
    from eigenface.distributed import pack_keys
    out = np.full(len(pairs), N.EF_KEY_NONE, np.int64)
    for j, p in enumerate(pairs):
        if p is not None:
            v = -p[0] if metric == "cosine" else p[0]
            out[j] = pack_keys(np.array([v], np.float32), np.array([p[1]]))[0]
    return out


# six probes: (genuine, impostor) as (score, row)
#   0 correct          1 wrong rank 1       2 no genuine row (not enrolled twice)
#   3 no impostor row  4 equal scores, genuine row lower: correct   5 equal scores, impostor row lower: wrong
COSINE = dict(genuine=[(0.875, 10), (0.5, 11), None, (0.75, 13), (0.625, 5), (0.625, 9)],
              impostor=[(0.5, 20), (0.75, 21), (0.625, 22), None, (0.625, 9), (0.625, 5)],
              thresholds=[0.5, 0.625, 0.75, 0.875],
              # 5 probes have a genuine row; rank-1 correct: 0, 3, 4 with similarities 0.875, 0.75, 0.625
              fnir=[0.4, 0.4, 0.6, 0.8],
              # 5 probes have an impostor row, similarities 0.5, 0.75, 0.625, 0.625, 0.625
              fpir=[1.0, 0.8, 0.2, 0.0],
              eer=0.75, tie=([0.7, 0.75], 0.75))
L2 = dict(genuine=[(1.0, 10), (4.0, 11), None, (2.0, 13), (3.0, 5), (3.0, 9)],
          impostor=[(4.0, 20), (2.0, 21), (3.0, 22), None, (3.0, 9), (3.0, 5)],
          thresholds=[1.0, 2.0, 3.0, 4.0],
          fnir=[0.8, 0.6, 0.4, 0.4],  # correct: 0, 3, 4 at distances 1, 2, 3
          fpir=[0.0, 0.2, 0.8, 1.0],  # impostor distances 4, 2, 3, 3, 3
          eer=2.0, tie=([2.0, 2.5], 2.0))


@pytest.mark.parametrize("metric,ex", [("cosine", COSINE), ("l2", L2)])
def test_open_set_rates_on_six_probes(metric, ex):
    from eigenface import equal_error_threshold, open_set_rates
    gk, ik = _keys(ex["genuine"], metric), _keys(ex["impostor"], metric)
    r = open_set_rates(gk, ik, metric)
    np.testing.assert_array_equal(r.thresholds, ex["thresholds"])  # sorted distinct finite scores
    np.testing.assert_allclose(r.fnir, ex["fnir"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(r.fpir, ex["fpir"], rtol=0, atol=1e-15)
    assert r.rank1 == 3 / 5
    assert equal_error_threshold(gk, ik, metric) == ex["eer"]
    cand, strict = ex["tie"]  # both candidates give max(FNIR, FPIR) = 0.6: the strictest wins
    rt = open_set_rates(gk, ik, metric, cand)
    np.testing.assert_allclose(np.maximum(rt.fnir, rt.fpir), [0.6, 0.6], rtol=0, atol=1e-15)
    assert equal_error_threshold(gk, ik, metric, cand) == strict


def test_rates_without_one_side_are_nan():
    from eigenface import _native as N, equal_error_threshold, open_set_rates
    gk = _keys([(0.9, 1), (0.8, 0)], "cosine")
    none = np.full(2, N.EF_KEY_NONE, np.int64)
    r = open_set_rates(gk, none, "cosine")
    assert r.rank1 == 1.0 and np.isnan(r.fpir).all() and not np.isnan(r.fnir).any()
    assert equal_error_threshold(gk, none, "cosine") == np.float32(0.8)  # FNIR alone: 0 up to the lowest genuine
    r = open_set_rates(none, gk, "cosine")
    assert np.isnan(r.rank1) and np.isnan(r.fnir).all()
    assert open_set_rates(none, none, "l2").thresholds.size == 0
    assert np.isnan(equal_error_threshold(none, none, "l2"))
    with pytest.raises(ValueError):
        open_set_rates(gk, none[:1], "cosine")
    with pytest.raises(ValueError):
        open_set_rates(gk, none, "dot")


def test_evaluate_model_with_one_label_has_nan_fpir():
    """One identity only: the impostor side is empty, FPIR is NaN, nothing raises; with the
    keys passed in no GPU path is touched."""
    from eigenface import _native as N, evaluate_model
    model = {"face_features": np.eye(4, 3, dtype=np.float32), "face_labels": ["ann"] * 4}
    gk = _keys([(0.75, 1), (0.75, 0), (0.5, 0), (0.875, 2)], "cosine")
    ik = np.full(4, N.EF_KEY_NONE, np.int64)
    out = evaluate_model(model, "cosine", keys=(gk, ik))
    assert out["rank1"] == 1.0 and out["n"] == 4
    assert sorted(out["at"]) == [0.7, 0.8]
    assert np.isnan(out["at"][0.7]["fpir"]) and np.isnan(out["at"][0.8]["fpir"]) and np.isnan(out["equal_error_fpir"])
    assert out["at"][0.7]["fnir"] == 0.25 and out["at"][0.8]["fnir"] == 0.75
    assert out["equal_error_threshold"] == 0.5 and out["equal_error_fnir"] == 0.0
    with pytest.raises(ValueError):
        evaluate_model(model, "cosine", keys=(gk[:3], ik[:3]))


def test_labelled_entry_points_are_bound():
    from eigenface import _native as N
    lib = N.lib()
    for name in ("ef_gallery_labels", "ef_search_labelled"):
        assert name in N._SIGS and name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert (N.EF_LABEL_SAME, N.EF_LABEL_OTHER, N.EF_LABEL_ANY) == (0, 1, 2)
    # a NULL context is refused before anything else
    assert lib.ef_gallery_labels(None, None, 0, 0) == N.EF_E_INVALID
    assert lib.ef_search_labelled(None, None, 0, 0, 0, None, None, None, None, 0) == N.EF_E_INVALID


def test_labelled_search_checks_inputs_before_the_c_call():
    from eigenface import Engine, _native as N
    e = object.__new__(Engine)
    e._lib, e._h = N.lib(), ctypes.c_void_p()
    e.model_d = e.model_k = e.gallery_k = None
    e.gallery_n = 0
    q = np.zeros((4, 8), np.float32)
    lab = np.zeros(4, np.int32)
    with pytest.raises(RuntimeError):
        e.search_labelled_keys(q, lab)
    with pytest.raises(RuntimeError):
        e.set_gallery_labels(lab)
    e.gallery_k = 8
    for bad_q in (np.zeros((4, 7), np.float32), np.zeros(8, np.float32)):
        with pytest.raises(ValueError):
            e.search_labelled_keys(bad_q, lab)
    with pytest.raises(ValueError):
        e.search_labelled_keys(q, lab[:3])
    with pytest.raises(ValueError):
        e.search_labelled_keys(q, lab, "same", np.zeros(5, np.int64))
    with pytest.raises(ValueError):
        e.search_labelled_keys(q, None, "same")
    with pytest.raises(KeyError):
        e.search_labelled_keys(q, lab, "nearest")
    with pytest.raises(ValueError):
        e.set_gallery_labels(np.zeros((4, 1), np.int32))
