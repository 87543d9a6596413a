"""Model bank distance from face space and face gate, the parts that need no GPU: the new entry
points are exported and bound, the grouped residual's plan (ef_bank_recon_schedule) keeps its
invariants, and the gated best-over-models rule equals a literal restatement of the walk of
scan-template-v4.py:293-309 with the gate's skip in it."""
import ctypes

import numpy as np
import pytest

NEW_SYMBOLS = ("ef_bank_recon_set", "ef_bank_face_distance", "ef_bank_recognize_gated", "ef_scan_frame_gated",
               "ef_bank_recon_schedule")
EF_E_INVALID = -1


def test_symbols_exported_and_bound_version_unchanged():
    from eigenface import _native
    lib = _native.lib()
    for n in NEW_SYMBOLS:
        assert n in _native.EXPORTED_SYMBOLS, n
        fn = getattr(lib, n)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, n
    assert lib.ef_api_version() == 7  # additive: detected by symbol, not by version
    from eigenface import Engine, FrameScanner, ModelBank, bank_recon_schedule, face_gate_mask  # noqa: F401
    for m in ("bank_set_reconstruction", "bank_face_distance", "bank_recognize_gated", "scan_frame_gated"):
        assert callable(getattr(Engine, m)), m
    for m in ("face_distance", "is_face"):
        assert callable(getattr(ModelBank, m)), m
    # a free flag bit
    flags = [_native.EF_FIT_STANDARDIZE, _native.EF_MODEL_BF16, _native.EF_MEM_DEVICE, _native.EF_IMG_RGB,
             _native.EF_ROI_RECTS_DEVICE, _native.EF_BANK_GATE_RELATIVE]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)


def _schedule(b, d, m):
    from eigenface import _native
    ns, tps, nwg, sb = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _native.lib().ef_bank_recon_schedule(b, d, m, ctypes.byref(ns), ctypes.byref(tps), ctypes.byref(nwg),
                                              ctypes.byref(sb))
    return rc, ns.value, tps.value, nwg.value, sb.value


@pytest.mark.parametrize("b", [1, 128, 129, 4096])
@pytest.mark.parametrize("d", [100, 4096, 16384])
@pytest.mark.parametrize("m", [1, 3, 64, 4096])
def test_bank_recon_schedule_invariants(b, d, m):
    rc, ns, tps, nwg, sb = _schedule(b, d, m)
    assert rc == 0
    assert 1 <= ns <= 64
    ntiles = -(-d // 128)
    assert tps >= 1 and ns * tps >= ntiles > (ns - 1) * tps  # covers every tile, no empty split
    ptiles = -(-b // 128)
    assert nwg == ptiles * m * ns
    assert sb == 2 * ns * m * ptiles * 128 * 4
    # the bank's split rule: about 512 workgroups wherever the caps (64, the tile count) allow it
    # (rounding the tiles per split up can only take splits away again)
    items = ptiles * m
    want = min(-(-512 // items), 64, ntiles)
    assert ns <= want and tps == -(-ntiles // want)
    if items >= 512:
        assert ns == 1


def test_bank_recon_schedule_regimes_and_dict_form():
    from eigenface import bank_recon_schedule
    assert bank_recon_schedule(1, 256, 600)["nsplit"] == 1
    assert bank_recon_schedule(1, 4096, 2) == {"nsplit": 32, "tiles_per_split": 1, "n_workgroups": 64,
                                                "scratch_bytes": 2 * 32 * 2 * 128 * 4}
    assert bank_recon_schedule(300, 4096, 5)["nsplit"] == 32  # capped at the tile count: 3 x 5 x 32 workgroups


def test_bank_recon_schedule_rejects_bad_arguments():
    assert _schedule(4097, 4096, 4)[0] == EF_E_INVALID
    assert _schedule(0, 4096, 4)[0] == EF_E_INVALID
    assert _schedule(8, 0, 4)[0] == EF_E_INVALID
    assert _schedule(8, -5, 4)[0] == EF_E_INVALID
    assert _schedule(8, 4096, 0)[0] == EF_E_INVALID
    assert _schedule(8, 4096, 4097)[0] == EF_E_INVALID
    assert _schedule(8, 4096, 4096)[0] == 0
    from eigenface import EigenfaceError, _native, bank_recon_schedule
    assert _native.lib().ef_bank_recon_schedule(8, 4096, 4, None, None, None, None) == 0  # every output is optional
    with pytest.raises(EigenfaceError):
        bank_recon_schedule(8, 4096, 0)


def _gated_walk(scores, allowed, l2):
    """scan-template-v4.py:293-309 for one face with the gate's skip: `scores` in model order
    (None = no gallery row), a model that is not allowed is passed over."""
    best_result = None
    best_value = -np.inf if l2 else 0.0
    for slot, s in enumerate(scores):
        if s is None or not allowed[slot]:
            continue
        value = -s if l2 else s
        if value > best_value:
            best_value = value
            best_result = slot
    return best_result if best_result is not None else -1


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_best_over_models_allowed_is_the_gated_walk(metric):
    from eigenface import best_over_models
    l2 = metric == "l2"
    rng = np.random.default_rng(21)
    s = rng.uniform(-1, 1, (300, 7)).astype(np.float32)
    if l2:
        s = np.abs(s) * 9
    s[rng.random(s.shape) < 0.15] = np.nan  # empty slots
    s[:60] = np.round(s[:60], 1)            # many equal extrema
    ok = rng.random(s.shape) < 0.6
    ok[100:110] = False
    ok[110:120] = True
    got = best_over_models(s, metric, allowed=ok)
    want = [_gated_walk([None if np.isnan(v) else float(v) for v in row], a, l2) for row, a in zip(s, ok)]
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32
    # all true: the ungated result, which is also the default's; all false: nobody
    np.testing.assert_array_equal(best_over_models(s, metric, allowed=np.ones_like(ok)), best_over_models(s, metric))
    np.testing.assert_array_equal(best_over_models(s, metric, allowed=None), best_over_models(s, metric))
    assert (best_over_models(s, metric, allowed=np.zeros_like(ok)) == -1).all()
    assert (got[100:110] == -1).all()
    np.testing.assert_array_equal(got[110:120], best_over_models(s, metric)[110:120])
    # a winner that is masked hands the face to the next best allowed model
    row = np.array([[0.5, 0.9, 0.7]], np.float32)
    if l2:
        assert best_over_models(row, "l2", allowed=[[False, True, True]]).tolist() == [2]
    else:
        assert best_over_models(row, "cosine", allowed=[[True, False, True]]).tolist() == [2]
    # NaN scores never win, allowed or not
    assert best_over_models(np.full((2, 3), np.nan, np.float32), metric, allowed=np.ones((2, 3), bool)).tolist() == [-1, -1]
    with pytest.raises(ValueError):
        best_over_models(s, metric, allowed=ok[:, :-1])


def test_face_gate_mask_is_the_fp32_comparison():
    from eigenface import face_gate_mask
    inf, nan = np.inf, np.nan
    eps2 = np.array([[1.0, 1.0, 1.0, nan, 5.0, 0.0]], np.float32)
    en = np.array([[10.0, 10.0, 0.0, 10.0, nan, 0.0]], np.float32)
    gate = np.array([0.2, 0.05, inf, 0.1, 0.1, 0.0], np.float32)
    # relative: 1 > 2 no; 1 > 0.5 yes; inf * 0 = NaN -> no; NaN > 1 no; 5 > NaN no; 0 > 0 no
    np.testing.assert_array_equal(face_gate_mask(eps2, en, gate), [[True, False, True, True, True, True]])
    # absolute: 1 > 0.2, 1 > 0.05, 1 > inf no, NaN no, 5 > 0.1, 0 > 0 no
    np.testing.assert_array_equal(face_gate_mask(eps2, en, gate, relative=False),
                                  [[False, False, True, True, False, True]])
    assert face_gate_mask(eps2, en, np.full(6, nan, np.float32)).all()
    # one fp32 multiply: a bound that differs between fp32 and fp64 arithmetic
    g, e = np.float32(0.1), np.float32(3.0)
    b32 = g * e
    assert float(b32) != float(g) * float(e)
    assert bool(face_gate_mask([[b32]], [[e]], [g])[0, 0])
    assert not bool(face_gate_mask([[np.nextafter(b32, np.float32(1))]], [[e]], [g])[0, 0])
