"""Model bank, the parts that need no GPU: the five entry points are exported and bound, the
grouped projection's plan (ef_bank_schedule) keeps its invariants, and the best-over-models rule
used for labelling equals a literal restatement of scan-template-v4.py:293-319."""
import ctypes

import numpy as np
import pytest

BANK_SYMBOLS = ("ef_bank_clear", "ef_bank_add", "ef_bank_info", "ef_bank_recognize", "ef_bank_schedule")
EF_E_INVALID = -1


def test_bank_symbols_exported_and_bound_version_unchanged():
    from eigenface import _native
    lib = _native.lib()
    for n in BANK_SYMBOLS:
        assert n in _native.EXPORTED_SYMBOLS, n
        fn = getattr(lib, n)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, n
    assert lib.ef_api_version() == 7  # additive: detected by symbol, not by version
    from eigenface import Engine, ModelBank, best_over_models  # noqa: F401
    for m in ("bank_clear", "bank_add", "bank_info", "bank_recognize"):
        assert callable(getattr(Engine, m))
    assert _native.EF_BANK_MAX_MODELS == 4096 and _native.EF_BANK_MAX_PROBES == 4096


def _schedule(b, d, ks):
    from eigenface import _native
    k = np.asarray(ks, np.int32)
    ns, pps, nwg, sb = ctypes.c_int32(-1), ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _native.lib().ef_bank_schedule(b, d, k.ctypes.data if len(k) else None, len(k), ctypes.byref(ns),
                                        ctypes.byref(pps), ctypes.byref(nwg), ctypes.byref(sb))
    return rc, ns.value, pps.value, nwg.value, sb.value


def _kp(k):
    for p in (16, 32, 64, 128, 256, 512):
        if k <= p:
            return p
    return -(-k // 128) * 128


@pytest.mark.parametrize("b", [1, 128, 129, 4096])
@pytest.mark.parametrize("d", [100, 4096])
@pytest.mark.parametrize("ks", [[3], [64, 65, 130, 520], [200] * 300, [65536], [1] * 4096])
def test_bank_schedule_invariants(b, d, ks):
    rc, ns, pps, nwg, sb = _schedule(b, d, ks)
    assert rc == 0
    assert 1 <= ns <= 64
    assert pps % 32 == 0 and pps > 0
    assert ns * pps >= d > (ns - 1) * pps
    ptiles = -(-b // 128)
    coltiles = sum(-(-_kp(k) // 128) for k in ks)
    assert nwg == ptiles * coltiles * ns
    # the split is capped at the number of 32-pixel stages
    assert ns <= -(-d // 32)
    # partial slabs + padded feature blocks, fp32
    assert sb == (ns * coltiles * 128 + sum(_kp(k) for k in ks)) * ptiles * 128 * 4


def test_bank_schedule_keeps_the_launch_near_a_few_workgroups_per_cu():
    """The rule itself: about 2-4 workgroups per CU (256 CUs) wherever the caps allow it."""
    for b, d, ks in [(8, 4096, [600] * 50), (1, 4096, [100] * 8), (64, 4096, [600] * 64), (1, 4096, [600] * 8)]:
        rc, ns, pps, nwg, _ = _schedule(b, d, ks)
        assert rc == 0
        items = nwg // ns
        if items >= 1024:
            assert ns == 1
        elif ns < 64:
            assert 512 <= nwg <= 1024 + items, (b, ks[0], len(ks), ns, nwg)


def test_bank_schedule_rejects_bad_arguments():
    assert _schedule(4097, 4096, [16])[0] == EF_E_INVALID
    assert _schedule(0, 4096, [16])[0] == EF_E_INVALID
    assert _schedule(8, 0, [16])[0] == EF_E_INVALID
    assert _schedule(8, 4096, [16, 0])[0] == EF_E_INVALID
    assert _schedule(8, 4096, [-3])[0] == EF_E_INVALID
    assert _schedule(8, 4096, [65537])[0] == EF_E_INVALID
    assert _schedule(8, 4096, [])[0] == EF_E_INVALID
    assert _schedule(8, 4096, [16] * 4097)[0] == EF_E_INVALID
    assert _schedule(8, 4096, [16] * 4096)[0] == 0
    from eigenface import _native
    k = np.array([16], np.int32)  # every output is optional
    assert _native.lib().ef_bank_schedule(8, 4096, k.ctypes.data, 1, None, None, None, None) == 0


def _reference_walk(scores):
    """scan-template-v4.py:293-319 for one face, literally: `scores` are the confidences the
    models return in iteration order (None = the model raised or has no gallery)."""
    best_result = None
    best_confidence = 0.0
    for slot, confidence in enumerate(scores):
        if confidence is None:
            continue
        if confidence > best_confidence:
            best_confidence = confidence
            best_result = slot
    return best_result if best_result is not None else -1


def test_best_over_models_is_the_reference_walk():
    from eigenface import best_over_models
    rng = np.random.default_rng(11)
    s = rng.uniform(-1, 1, (200, 7)).astype(np.float32)
    s[rng.random(s.shape) < 0.15] = np.nan  # empty slots
    s[:40] = np.round(s[:40], 1)            # many equal maxima
    s[40:60] = -np.abs(s[40:60])            # nothing above 0
    s[60, :] = 0.0
    s[61, :] = np.nan
    s[62] = [0.5, 0.7, 0.7, 0.2, 0.7, -1, np.nan]
    got = best_over_models(s, "cosine")
    want = [_reference_walk([None if np.isnan(v) else float(v) for v in row]) for row in s]
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32
    assert got[62] == 1 and got[60] == -1 and got[61] == -1 and (got[40:60] == -1).all()
    assert best_over_models(np.zeros((3, 0), np.float32)).tolist() == [-1, -1, -1]
    assert best_over_models(np.zeros((0, 4), np.float32)).shape == (0,)


def test_best_over_models_l2_first_smallest_distance():
    from eigenface import best_over_models
    s = np.array([[3.0, 1.0, 1.0, 2.0], [np.nan, 5.0, np.nan, 4.0], [np.nan] * 4, [0.0, 0.0, 7.0, 0.0],
                  [np.inf, np.inf, np.inf, np.inf]], np.float32)
    np.testing.assert_array_equal(best_over_models(s, "l2"), [1, 3, -1, 0, -1])
    rng = np.random.default_rng(12)
    t = np.round(rng.uniform(0, 9, (100, 6)), 0).astype(np.float32)
    np.testing.assert_array_equal(best_over_models(t, "l2"), np.argmin(t, axis=1))
