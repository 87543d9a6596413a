"""Host side of the top-m search (no GPU): ef_matches_merge_topk with ctx = NULL and its
Python wrapper merge_topk_host, against the rule of include/eigenface.h — rank 0 is the lowest
global index among the records within 1e-12 (|min| + max scale) of the minimum, the others
follow in (score, global index) order, EF_KEY_NONE records are skipped and missing ranks are
padded."""
import ctypes as C

import numpy as np
import pytest

from eigenface import _native as N
from eigenface import merge_matches_host, merge_topk_host
from eigenface.distributed import make_matches, pack_keys

NONE = N.EF_KEY_NONE


def _parts(scores, idx, scale=1.0):
    """scores / idx (nparts, b, m) -> records (nparts, b, m); +inf score = empty slot."""
    scores = np.asarray(scores, np.float64)
    rec = make_matches(scores.reshape(-1), scale, np.asarray(idx).reshape(-1))
    return rec.reshape(scores.shape)


def _rows(keys):
    k = np.asarray(keys)
    return np.where(k == NONE, -1, k & 0xFFFFFFFF)


def _merge_c(parts, b, m, merged=False):
    """The raw C call with ctx = NULL."""
    lib = N.lib()
    p = np.ascontiguousarray(parts).reshape(-1)
    nparts = len(p) // (b * m)
    keys = np.empty((b, m), np.int64)
    out = np.empty((b, m), N.MATCH_DTYPE) if merged else None
    rc = lib.ef_matches_merge_topk(None, p.ctypes.data, nparts, b, m, keys.ctypes.data,
                                   out.ctypes.data if merged else None, 0)
    assert rc == N.EF_OK
    return (keys, out) if merged else keys


def test_symbols_bound_and_api_version():
    lib = N.lib()
    for name in ("ef_search_topk", "ef_recognize_topk", "ef_search_topk_matches", "ef_matches_merge_topk",
                 "ef_search_topk_stats"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.ef_api_version() == 7
    assert N.EF_OPT_SEARCH_TOPK_CAND == 12


def test_fp64_scores_order_what_fp32_keys_cannot():
    # two shards whose rank-0 rows round to the same fp32 score; the fp64 scores say row 900 wins
    a, bb = 1.0 + 3e-9, 1.0 + 1e-9
    assert np.float32(a) == np.float32(bb)
    parts = _parts([[[a, 2.0]], [[bb, 1.5]]], [[[7, 8]], [[900, 901]]])
    keys = merge_topk_host(parts, 1, 2)
    assert _rows(keys).tolist() == [[900, 7]]
    np.testing.assert_array_equal(keys, _merge_c(parts, 1, 2))
    # a MIN over the fp32 keys would have taken the lower index
    assert min(parts["key"][0, 0, 0], parts["key"][1, 0, 0]) & 0xFFFFFFFF == 7


def test_tie_window_goes_to_lowest_index_rest_in_score_index_order():
    s = 4.0
    tie = s * (1 + 2e-13)  # inside 1e-12 (|min| + scale), scale = 1
    out = s * (1 + 1e-11)  # outside
    # part 0 holds rows 50 (tie, not the minimum) and 60; part 1 rows 10 (outside), 70 (minimum), 71 (= 60's score)
    parts = _parts([[[tie, 5.0, np.inf]], [[s, out, 5.0]]], [[[50, 60, 0]], [[70, 10, 71]]])
    keys, merged = _merge_c(parts, 1, 3, merged=True)
    # rank 0: rows 50 and 70 are in the window -> 50; then (score, index): 70 (s), 10 (out)
    assert _rows(keys).tolist() == [[50, 70, 10]]
    assert merged["score"][0].tolist() == [tie, s, out]
    assert (merged["scale"] == 1.0).all() and (merged["key"] == keys).all()
    # equal scores in different parts: ascending global index
    parts = _parts([[[1.0, 5.0, 6.0]], [[2.0, 5.0, 7.0]]], [[[3, 60, 61]], [[4, 59, 62]]])
    assert _rows(merge_topk_host(parts, 1, 3)).tolist() == [[3, 4, 59]]


def test_none_records_are_skipped_and_short_results_padded():
    inf = np.inf
    parts = _parts([[[1.0, inf, inf], [inf, inf, inf]], [[inf, inf, inf], [inf, inf, inf]], [[0.5, 3.0, inf], [inf, inf, inf]]],
                   [[[5, 0, 0], [0, 0, 0]], [[0, 0, 0], [0, 0, 0]], [[9, 2, 0], [0, 0, 0]]])
    keys, merged = _merge_c(parts, 2, 3, merged=True)
    assert _rows(keys).tolist() == [[9, 5, 2], [-1, -1, -1]]
    assert np.isinf(merged["score"][1]).all() and (merged["scale"][1] == 0).all() and (merged["key"][1] == NONE).all()
    # fewer records than m
    parts = _parts([[[2.0, inf, inf, inf]], [[1.0, inf, inf, inf]]], [[[1, 0, 0, 0]], [[0, 0, 0, 0]]])
    assert _rows(merge_topk_host(parts, 1, 4)).tolist() == [[0, 1, -1, -1]]


def test_one_part_is_the_identity():
    rng = np.random.default_rng(3)
    b, m = 17, 6
    scores = np.sort(rng.random((1, b, m)) + 1.0, axis=2)
    scores[0, 3, 4:] = np.inf
    idx = rng.permutation(b * m).reshape(1, b, m)
    parts = _parts(scores, idx, scale=2.0)
    keys, merged = _merge_c(parts, b, m, merged=True)
    np.testing.assert_array_equal(keys, parts["key"][0])
    np.testing.assert_array_equal(merged["score"], parts["score"][0])
    # the int64 view is accepted too
    np.testing.assert_array_equal(merge_topk_host(parts.view(np.int64).reshape(-1, 3), b, m), keys)


def test_m1_equals_matches_merge():
    rng = np.random.default_rng(4)
    nparts, b = 5, 200
    scores = np.round(rng.random((nparts, b, 1)) * 8) / 8 + 1.0  # many exact ties
    scores[rng.random((nparts, b, 1)) < 0.2] = np.inf
    scores[:, 0] = np.inf  # a probe with no record at all
    scores[:, 1] *= 1 + 5e-13 * np.arange(nparts)[:, None]  # inside the window
    idx = rng.permutation(nparts * b).reshape(nparts, b, 1)
    parts = _parts(scores, idx, scale=rng.random((nparts * b)) + 1.0)
    keys = merge_topk_host(parts, b, 1)
    np.testing.assert_array_equal(keys[:, 0], merge_matches_host(parts.reshape(-1), b))
    assert keys[0, 0] == NONE


def test_bad_arguments_are_rejected():
    lib = N.lib()
    parts = _parts([[[1.0]]], [[[0]]])
    keys = np.empty(64, np.int64)
    for b, m in ((1, 0), (1, 65), (-1, 1)):
        assert lib.ef_matches_merge_topk(None, parts.ctypes.data, 1, b, m, keys.ctypes.data, None, 0) != N.EF_OK
    assert lib.ef_matches_merge_topk(None, None, 1, 1, 1, keys.ctypes.data, None, 0) != N.EF_OK
    assert lib.ef_matches_merge_topk(None, parts.ctypes.data, 1, 1, 1, keys.ctypes.data, None, N.EF_MEM_DEVICE) != N.EF_OK
    for b, m in ((1, 0), (1, 65), (-1, 1), (2, 1)):
        with pytest.raises(ValueError):
            merge_topk_host(parts, b, m)
    assert merge_topk_host(np.empty(0, N.MATCH_DTYPE), 0, 3).shape == (0, 3)


def test_keys_carry_the_fp32_score_of_the_fp64_record():
    parts = _parts([[[0.0, 1.0 + 1e-9]], [[-0.0, 3.0]]], [[[4, 5]], [[2, 6]]])
    keys = merge_topk_host(parts, 1, 2)
    np.testing.assert_array_equal(keys[0], pack_keys(np.float32([0.0, 0.0]), [2, 4]))
    assert isinstance(C.sizeof(N.ef_match), int) and C.sizeof(N.ef_match) == 24
