"""Every route through the one search path gives the answer of the fp64 rule.

The host layer plans, stages and launches every search mode from one copy of each step (one
planner, one scan selector, one top-1 sequence, one gallery loader).  This file walks the
routes: per feature width the scan variants of EF_OPT_SEARCH_SPLIT_BF16, the prefix scan in
both arithmetics, top-1 and top-m, keys and match records, host arrays and device tensors —
all on one small gallery with planted duplicates and ties, against parity_util (top-1) and
topk_util (top-m) on the fp64 scores of the same fp32 features.
"""
import numpy as np
import pytest
import torch

from eigenface import EigenfaceError, decode_keys
from eigenface import _native as N
from parity_util import assert_exact_argbest, top2
from topk_util import Reference, check_topk

pytestmark = pytest.mark.gpu

NONE = N.EF_KEY_NONE
METRICS = ("l2", "cosine")
N_ROWS = 193   # three 64-row tiles and one row
B = 257        # one full probe tile and one row
OFFSET = 1000  # global index of gallery row 0
M = 3
K1 = 16        # forced prefix length
DUP_PROBES = (0, 64, 128, 192, 5)    # gallery rows copied into probes 0 .. 4
TIED_ROWS = ((5, 100), (64, 65), (7, 192))  # (first, second): the second row is a copy of the first


@pytest.fixture
def e(eng):
    """The session engine with the search options at their defaults before and after."""
    def reset():
        eng.set_option("search_split_bf16", 0)
        eng.set_option("search_prefix", 1)
        eng.set_option("search_prefix_split", 1)
        eng.set_option("search_topk_cand", 1024)
    reset()
    yield eng
    reset()


def _data(k):
    rng = np.random.default_rng(7000 + k)
    g = rng.standard_normal((N_ROWS, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    for a, c in TIED_ROWS:
        g[c] = g[a]  # exact ties between two gallery rows
    for p, r in enumerate(DUP_PROBES):
        q[p] = g[r]  # exact duplicates of gallery rows (rows 5 and 64 are tied rows too)
    for p, (a, _) in enumerate(TIED_ROWS):
        q[10 + p] = g[a] + np.float32(1e-3) * rng.standard_normal(k).astype(np.float32)  # near a tied pair
    return g, q


def _rows(keys):
    k = np.asarray(keys)
    return np.where(k == NONE, -1, (k & 0xFFFFFFFF) - OFFSET)


def _calls(e, q, metric, prefix):
    """The four calls on host arrays and on device tensors: {name: (host result, device result)},
    records as (.., 3) int64 either way, and the search_stats of the four top-1 searches.  Setting
    search_prefix clears the guard, so it is set again before each of them: every one decides
    alone whether the prefix scan runs, whatever the one before sent to the full-k scan."""
    qd = torch.as_tensor(q).cuda()
    out, stats = {}, []

    def top1(fn, x):
        e.set_option("search_prefix", prefix)
        r = fn(x, metric)
        stats.append(e.search_stats())
        return r

    out["keys"] = (top1(e.search_keys, q), top1(e.search_keys, qd).cpu().numpy())
    out["matches"] = (top1(e.search_matches, q), top1(e.search_matches, qd).cpu().numpy())
    out["topk_keys"] = (e.search_topk_keys(q, M, metric), e.search_topk_keys(qd, M, metric).cpu().numpy())
    out["topk_matches"] = (e.search_topk_matches(q, M, metric), e.search_topk_matches(qd, M, metric).cpu().numpy())
    for name in ("matches", "topk_matches"):
        h, d = out[name]
        out[name] = (np.ascontiguousarray(h).view(np.int64).reshape(h.shape + (3,)), d)
    return out, stats


@pytest.mark.parametrize("k", [13, 128, 200, 600])
def test_every_route_gives_the_fp64_answer(e, k):
    g, q = _data(k)
    kp = {13: 16, 128: 128, 200: 256, 600: 640}[k]
    e.set_gallery(g, global_offset=OFFSET)
    for metric in METRICS:
        ref1 = top2(q, g, metric)
        refm = Reference(q, g, metric, ranks=M)
        for split in (0, 1, 2, 3):
            for prefix in (0, K1):
                if prefix >= kp:
                    continue  # the setter refuses a prefix that is no shorter than the padded k
                for prefix_split in (0, 1):
                    e.set_option("search_split_bf16", split)
                    e.set_option("search_prefix_split", prefix_split)
                    what = (k, metric, split, prefix, prefix_split)
                    res, stats = _calls(e, q, metric, prefix)
                    # the prefix scan runs exactly where it is legal: L2, fp32 scan, k1 < kp <= 128
                    legal = metric == "l2" and split == 0 and prefix and kp <= 128
                    for st in stats:  # host and device keys, host and device records
                        assert st[0] == B, what
                        assert (st[1] + st[2] == B) == bool(legal), (what, st)
                    for name, (h, d) in res.items():
                        np.testing.assert_array_equal(h, d, err_msg=f"{name} host != device {what}")
                    keys, rec = res["keys"][0], res["matches"][0]
                    tkeys, trec = res["topk_keys"][0], res["topk_matches"][0]
                    assert keys.shape == (B,) and rec.shape == (B, 3) and tkeys.shape == (B, M) and trec.shape == (B, M, 3)
                    idx = _rows(keys)
                    assert ((idx >= 0) & (idx < N_ROWS)).all(), what
                    assert_exact_argbest(q, g, idx, metric, ref=ref1)
                    check_topk(refm, M, _rows(tkeys))
                    np.testing.assert_array_equal(tkeys[:, 0], keys, err_msg=f"rank 0 {what}")
                    np.testing.assert_array_equal(rec[:, 2], keys, err_msg=f"record key {what}")
                    np.testing.assert_array_equal(trec[:, :, 2], tkeys, err_msg=f"top-m record key {what}")
                    # exact ties resolve to the first row
                    for p, r in enumerate(DUP_PROBES):
                        first = min([r] + [a for a, c in TIED_ROWS if c == r])
                        assert idx[p] == first, (what, p, idx[p])
                        twin = [c for a, c in TIED_ROWS if a == first]
                        if twin:
                            assert _rows(tkeys)[p, 1] == twin[0], (what, p)


def test_empty_gallery_gives_no_key_on_every_route(e):
    k = 13
    q = np.random.default_rng(1).standard_normal((B, k)).astype(np.float32)
    e.set_gallery(np.zeros((0, k), np.float32), global_offset=OFFSET)
    for metric in METRICS:
        for split in (0, 1):
            e.set_option("search_split_bf16", split)
            res, stats = _calls(e, q, metric, 1)
            for st in stats:
                assert st[0] == B and st[1] == 0 and st[2] == 0
            for name in ("keys", "topk_keys"):
                for r in res[name]:
                    assert (r == NONE).all(), (name, metric, split)
            for name in ("matches", "topk_matches"):
                for r in res[name]:
                    assert (r[..., 2] == NONE).all(), (name, metric, split)


def test_search_after_a_failed_gallery_load(e):
    g, q = _data(13)
    with pytest.raises(EigenfaceError, match="k > 65536"):
        e.set_gallery(np.zeros((1, 65537), np.float32))
    e.set_gallery(g, global_offset=OFFSET)
    for metric in METRICS:
        idx = _rows(e.search_keys(q, metric))
        assert_exact_argbest(q, g, idx, metric)
        check_topk(Reference(q, g, metric, ranks=M), M, _rows(e.search_topk_keys(q, M, metric)))


def test_bank_after_a_failed_add(e):
    rng = np.random.default_rng(11)
    d, b, ks, ns = 24, 5, (5, 40), (3, 70)
    mean = [rng.uniform(0, 255, d).astype(np.float32) for _ in ks]
    W = [rng.standard_normal((d, k)).astype(np.float32) for k in ks]
    G = [(20 * rng.standard_normal((n, k))).astype(np.float32) for n, k in zip(ns, ks)]
    P = rng.integers(0, 256, (b, d), dtype=np.uint8)
    e.bank_clear()
    try:
        assert e.bank_add(mean[0], W[0], G[0]) == 0
        with pytest.raises(EigenfaceError, match="k > 65536"):
            e.bank_add(mean[0], np.zeros((d, 65537), np.float32), np.zeros((1, 65537), np.float32))
        assert e.bank_info() == (1, d, ks[0], ns[0])  # the bank is unchanged
        assert e.bank_add(mean[1], W[1], G[1]) == 1
        assert e.bank_info() == (2, d, sum(ks), sum(ns))
        for metric in METRICS:
            idx, score, best, feats = e.bank_recognize(P, metric, return_features=True)
            assert idx.shape == (b, 2) and best.shape == (b,)
            for m in range(2):
                c64 = P.astype(np.float64) - mean[m].astype(np.float64)
                f64 = c64 @ W[m].astype(np.float64)
                # fp32 products summed in fp32, in any order: d roundings of at most 2^-23 of the terms' sum
                bound = d * 2.0 ** -23 * (np.abs(c64) @ np.abs(W[m].astype(np.float64)))
                assert (np.abs(feats[m] - f64) <= bound).all(), (metric, m)
                # the slot's arg-best is exact on the features the bank itself produced
                assert_exact_argbest(feats[m], G[m], idx[:, m], metric)
            want = np.nanargmin(score, axis=1) if metric == "l2" else np.nanargmax(score, axis=1)
            np.testing.assert_array_equal(score[np.arange(b), best], score[np.arange(b), want])
            keys_d = e.bank_recognize_raw(torch.as_tensor(P).cuda(), metric)[0].cpu().numpy()
            np.testing.assert_array_equal(keys_d, e.bank_recognize_raw(P, metric)[0])
    finally:
        e.bank_clear()
