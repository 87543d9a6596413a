"""The exact arg-best guarantee off unit scale.

Every search mode promises the fp64 first-arg-best outside the tie window (include/eigenface.h,
DESIGN.md "Exact arg-best").  The other search tests use unit-scale Gaussian features, where the
scan's own fp32 / bf16 scores already pick the right row; here the inputs make those scores
useless or push them to fp32's exponent limits, so the answer rests on the error bound
(scan_delta), its domain check (scan_regular), the COLLECT pass and the fp64 sweeps.

* conditioning: parity_util's offset_cluster / norm_outlier / dominant_component on every route;
  tests/test_parity_generators_cpu.py shows on the fp64 reference alone that >= 95 % of the probes
  are outside the tie window and that a plain fp32 scan picks the wrong row for 44 % .. 100 % of
  the offset-1000 probes;
* the exponent range: the unit-scale data of test_gpu_search_paths times 2^s, up to and past the
  points where fp32 norms overflow, turn subnormal and vanish;
* NaN and infinite components in a gallery row or a probe (last in the file).
"""
import numpy as np
import pytest
import torch

import labelled_util as lu
import parity_util as pu
import test_gpu_search_paths as paths
from eigenface import _native as N
from topk_util import Reference, check_topk

pytestmark = pytest.mark.gpu

NONE = N.EF_KEY_NONE
METRICS = ("l2", "cosine")
OFFSET = 1000  # global index of gallery row 0
M = 3
K1 = 16
KP = {13: 16, 128: 128, 200: 256, 600: 640}


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


def _rows(keys):
    k = np.asarray(keys)
    return np.where(k == NONE, -1, (k & 0xFFFFFFFF) - OFFSET)


def _as_int64(rec):
    """Host match records as the (.., 3) int64 a device call returns."""
    return np.ascontiguousarray(rec).view(np.int64).reshape(rec.shape + (3,))


def _fp64_scores(q, g, idx, metric):
    """fp64 score of row idx[p] for probe p as the records carry it: L2 the squared distance in
    difference form, cosine -cos."""
    return pu.l2_scores_diff(q, g, idx) if metric == "l2" else pu.chosen_scores(q, g, idx, metric)


def _routes(kp, metric):
    """(split, prefix, prefix_split) of every distinct route: the four scan variants, and the
    prefix scan in both arithmetics where it is legal (L2, fp32 scan, k1 < kp <= 128)."""
    for split in (0, 1, 2, 3):
        yield split, 0, 1
        if metric == "l2" and split == 0 and K1 < kp <= 128:
            yield split, K1, 0
            yield split, K1, 1


def _top1(e, q, qd, metric, prefix):
    """keys and records, host and device, each with the prefix guard cleared first."""
    out = []
    for fn, x in ((e.search_keys, q), (e.search_keys, qd), (e.search_matches, q), (e.search_matches, qd)):
        e.set_option("search_prefix", prefix)
        out.append(fn(x, metric))
    keys, keys_d, rec, rec_d = out
    np.testing.assert_array_equal(keys, keys_d.cpu().numpy(), err_msg="keys host != device")
    np.testing.assert_array_equal(_as_int64(rec), rec_d.cpu().numpy(), err_msg="records host != device")
    return keys, rec


def _check_top1(q, g, metric, keys, rec, ref1, what, min_clear=None):
    idx = _rows(keys)
    assert ((idx >= 0) & (idx < len(g))).all(), what
    clear = pu.assert_exact_argbest(q, g, idx, metric, ref=ref1, min_clear=min_clear)
    np.testing.assert_array_equal(rec["key"], keys, err_msg=f"record key {what}")
    want = _fp64_scores(q, g, idx, metric)
    assert (np.abs(rec["score"] - want) <= 1e-12 * np.abs(want)).all(), f"record score {what}"
    return idx, clear


def _check_topm(e, q, qd, metric, refm, keys, what):
    for cand in (1024, 16):  # 16: every list overflows its first round
        e.set_option("search_topk_cand", cand)
        tkeys = e.search_topk_keys(q, M, metric)
        np.testing.assert_array_equal(tkeys, e.search_topk_keys(qd, M, metric).cpu().numpy(),
                                      err_msg=f"top-m host != device {what} cand {cand}")
        check_topk(refm, M, _rows(tkeys))
        np.testing.assert_array_equal(tkeys[:, 0], keys, err_msg=f"rank 0 {what} cand {cand}")
    e.set_option("search_topk_cand", 1024)
    return e.topk_stats()


def _walk(e, g, q, k, min_clear=None):
    """Every route on one gallery: top-1 keys and records, top-m with and without overflow, the
    labelled search for both relations."""
    n = len(g)
    e.set_gallery(g, global_offset=OFFSET)
    glab = (np.arange(n) % 7).astype(np.int32)
    e.set_gallery_labels(glab)
    qd = torch.as_tensor(q).cuda()
    for metric in METRICS:
        ref1 = pu.top2(q, g, metric)
        refm = Reference(q, g, metric, ranks=M)
        for split, prefix, prefix_split in _routes(KP[k], metric):
            what = (k, n, metric, split, prefix, prefix_split)
            e.set_option("search_split_bf16", split)
            e.set_option("search_prefix_split", prefix_split)
            keys, rec = _top1(e, q, qd, metric, prefix)
            _check_top1(q, g, metric, keys, rec, ref1, what, min_clear)
            if prefix == 0:  # the top-m search has no prefix scan
                _check_topm(e, q, qd, metric, refm, keys, what)
        # labelled: the probe carries its nearest row's label and excludes that row
        e.set_option("search_split_bf16", 0)
        nearest = ref1[0]
        plab = glab[nearest]
        s = lu.score_matrix(q, g, metric)
        for rel in ("same", "other"):
            ref = lu.top2_masked(q, g, metric, glab, plab, rel, nearest, s=s)
            keys = e.search_labelled_keys(q, plab, rel, nearest + OFFSET, metric)
            keys_d = e.search_labelled_keys(qd, torch.as_tensor(plab).cuda(), rel,
                                            torch.as_tensor(nearest + OFFSET).cuda(), metric)
            np.testing.assert_array_equal(keys, keys_d.cpu().numpy(), err_msg=f"labelled host != device {rel}")
            lu.assert_labelled(q, g, metric, _rows(keys), ref)


@pytest.mark.parametrize("k", pu.CONDITIONING_KS)
@pytest.mark.parametrize("name", pu.CONDITIONING_GENERATORS)
def test_ill_conditioned_features_on_every_route(e, name, k):
    for n, b in pu.conditioning_shapes(k):
        g, q = pu.conditioning_case(name, n, b, k)
        _walk(e, g, q, k, min_clear=pu.MIN_CLEAR)


def test_the_hard_case_reaches_the_resolution_paths(e):
    """offset_cluster at c = 1000: the scan's scores are rounding noise (a plain fp32 argmin is
    wrong on 98 % of these probes, test_parity_generators_cpu.py), so the top-m search cannot
    finish every probe from its candidate lists."""
    k, n, b = 128, 3001, 300
    g, q = pu.conditioning_case("offset1000", n, b, k)
    e.set_gallery(g, global_offset=OFFSET)
    keys = e.search_keys(q, "l2")
    pu.assert_exact_argbest(q, g, _rows(keys), "l2", min_clear=pu.MIN_CLEAR)
    e.set_option("search_prefix", K1)
    pu.assert_exact_argbest(q, g, _rows(e.search_keys(q, "l2")), "l2")
    # The prefix scan can prove nothing here: its proof needs (prefix score of the runner-up) -
    # delta1 above the winner's full distance.  Prefix distances are ~ 2 K1 = 32 and full ones
    # ~ 2 k = 256, while delta1 = 4 (K1 + 4) u (2 |q| gm + gmax2) ~ 80 * 2^-24 * 3.8e8 ~ 1.8e3.
    probes, proven, full, _ = e.search_stats()
    assert probes == b and proven == 0 and full == b, (probes, proven, full)
    tkeys = e.search_topk_keys(q, M, "l2")
    check_topk(Reference(q, g, "l2", ranks=M), M, _rows(tkeys))
    st = e.topk_stats()
    assert st[0] == b and st[2] > 0, st  # probes resolved by the full fp64 sweep


# ------------------------------------------------------------------ the exponent range
def _scaled(x, s):
    return x * np.float32(2.0 ** s)  # exact: no element leaves fp32's normal range


@pytest.fixture(scope="module")
def unit_results(eng):
    """Per (k, metric): the engine's rows and record scores on the unscaled data, once."""
    cache = {}

    def get(k, metric):
        if (k, metric) not in cache:
            g, q = paths._data(k)
            eng.set_option("search_split_bf16", 0)
            eng.set_gallery(g, global_offset=OFFSET)
            rec = eng.search_matches(q, metric)
            cache[(k, metric)] = (_rows(rec["key"]), rec["score"].copy())
        return cache[(k, metric)]
    return get


@pytest.mark.parametrize("s", [-40, 40])
@pytest.mark.parametrize("k", [13, 128, 600])
def test_power_of_two_scaling_changes_nothing(e, unit_results, k, s):
    """2^s x is exact in fp32 and fp64, so the fp64 ranking is that of the unscaled data, every
    L2 score is 2^(2s) times the unscaled one and every cosine score is unchanged, bit for bit."""
    g0, q0 = paths._data(k)
    g, q = _scaled(g0, s), _scaled(q0, s)
    qd = torch.as_tensor(q).cuda()
    for metric in METRICS:
        idx0, score0 = unit_results(k, metric)
        e.set_gallery(g, global_offset=OFFSET)
        ref1 = pu.top2(q, g, metric)
        refm = Reference(q, g, metric, ranks=M)
        for split in (0, 1, 3):
            what = (k, s, metric, split)
            e.set_option("search_split_bf16", split)
            keys, rec = _top1(e, q, qd, metric, 1)
            idx, clear = _check_top1(q, g, metric, keys, rec, ref1, what)
            assert (idx[clear] == idx0[clear]).all(), what
            same = idx == idx0
            want = score0 * 4.0 ** s if metric == "l2" else score0
            np.testing.assert_array_equal(rec["score"][same], want[same], err_msg=f"scaled scores {what}")
            _check_topm(e, q, qd, metric, refm, keys, what)


def _norm2_f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return (x * x).sum(1, dtype=np.float32)


def _edge_exponents(g0, q0):
    """s chosen from the data.  Above: the largest s at which fp32 max ||g||^2 and max ||q||^2
    are still finite, then s + 1 and s + 3.  Below: the last s at which fp32 min ||g||^2 is
    normal, the first at which it is subnormal, the first at which it is 0, and the first at
    which every fp32 ||g||^2 is 0 (fully underflowed)."""
    tiny = np.finfo(np.float32).tiny
    hi = max(s for s in range(0, 70)
             if np.isfinite(_norm2_f32(_scaled(g0, s))).all() and np.isfinite(_norm2_f32(_scaled(q0, s))).all())
    down = range(0, -100, -1)
    sub = next(s for s in down if _norm2_f32(_scaled(g0, s)).min() < tiny)
    zero = next(s for s in down if _norm2_f32(_scaled(g0, s)).min() == 0)
    gone = next(s for s in down if _norm2_f32(_scaled(g0, s)).max() == 0)
    assert gone < zero < sub and np.all(_scaled(g0, gone)[g0 != 0] != 0)
    return (hi, hi + 1, hi + 3), (sub + 1, sub, zero, gone)


def test_edges_of_the_exponent_range(e):
    """All finite fp32 inputs have finite fp64 scores (k <= 65536), so the contract is the
    documented one with nothing taken off: the fp64 first-arg-best outside the tie window, and
    the record's score is the fp64 score.  Where fp32 squares overflow or underflow the scan's
    scores are +-inf, NaN or 0 and its error bound means nothing; scan_regular
    (csrc/ef_search_common.hpp) must send such probes to the fp64 sweeps.  Before that check
    existed a comparison with NaN or inf on one side read as "proven", and rows scoring +inf or
    NaN were never a chunk's best: at the first scale past the overflow point (L2, fp32 scan)
    this test failed on "every probe has a row of the gallery"."""
    k = 128
    g0, q0 = paths._data(k)
    above, below = _edge_exponents(g0, q0)
    for s in above + below:
        g, q = _scaled(g0, s), _scaled(q0, s)
        assert np.isfinite(g).all() and np.isfinite(q).all()
        qd = torch.as_tensor(q).cuda()
        e.set_gallery(g, global_offset=OFFSET)
        for metric in METRICS:
            ref1 = pu.top2(q, g, metric)
            refm = Reference(q, g, metric, ranks=M)
            assert np.isfinite(ref1[1]).all()
            for split in (0, 1):
                for prefix in (0, K1) if metric == "l2" and split == 0 else (0,):
                    what = (s, metric, split, prefix)
                    e.set_option("search_split_bf16", split)
                    keys, rec = _top1(e, q, qd, metric, prefix)
                    _check_top1(q, g, metric, keys, rec, ref1, what)
                _check_topm(e, q, qd, metric, refm, keys, what)


# ------------------------------------------------------------------ NaN and infinite values
BAD_ROWS = {3: (1, np.nan), 70: (0, np.inf), 150: (-1, -np.inf)}  # row: (column, value)
BAD_PROBES = {20: (1, np.nan), 100: (0, np.inf), 200: (-1, -np.inf), 256: (None, np.nan)}  # 256: every component


@pytest.mark.parametrize("k", [13, 600])
def test_non_finite_values_have_a_stated_behaviour(e, k):
    """What the search does with NaN and +-inf (include/eigenface.h, DESIGN.md "Exact arg-best"),
    read from the code before it was first run on them:

    * No index or address is formed from a score's value.  The scans take a block's arg-best
      from comparisons whose results pick a register number, COLLECT stores a row on
      `score <= threshold` (false for NaN), the candidate lists are read back under counts, and
      the sweeps walk rows 0 .. n - 1.
    * A gallery row with a NaN or an infinite component has an fp32 ||g||^2 that is not finite.
      gallery_aux_kernel flags the gallery, and every search on it skips the scan's verdict: each
      probe is re-scored against every row in fp64 (resolve_kernel's sweep, topk_sweep_kernel).
      Such a row scores NaN or +inf against a finite probe (score64: a NaN norm gives NaN, not
      the 0 of a zero vector) and is never below the minimum, so (ii)
      it is never returned, and max ||g||^2 (the tie window's scale) is taken over the other
      rows: (i) a finite probe's key and record are what they are on the gallery without those
      rows.
    * (iii) A probe with a NaN or an infinite component gets EF_KEY_NONE and the empty record
      (+inf, 0, EF_KEY_NONE), from reduce_kernel's fp64 ||q||^2, on every route and call; the
      probes that share its batch and tile are scanned in their own lanes and are unchanged.
    """
    g, q = paths._data(k)
    for r in BAD_ROWS:
        assert all(r not in pair for pair in paths.TIED_ROWS) and r not in paths.DUP_PROBES
    n, b = len(g), len(q)
    g_bad, q_bad = g.copy(), q.copy()
    for r, (c, v) in BAD_ROWS.items():
        g_bad[r, c] = v
    for p, (c, v) in BAD_PROBES.items():
        if c is None:
            q_bad[p, :] = v
        else:
            q_bad[p, c] = v
    fin = np.setdiff1d(np.arange(b), list(BAD_PROBES))
    kept = np.setdiff1d(np.arange(n), list(BAD_ROWS))
    qd_bad = torch.as_tensor(q_bad).cuda()
    for metric in METRICS:
        ref_clean = pu.top2(q[fin], g, metric)
        ref_kept = pu.top2(q[fin], g[kept], metric)
        for split in (0, 1):
            what = (k, metric, split)
            e.set_option("search_split_bf16", split)

            def run(gal, probes, probes_dev=None):
                e.set_gallery(gal, global_offset=OFFSET)
                pd = torch.as_tensor(probes).cuda() if probes_dev is None else probes_dev
                keys, rec = _top1(e, probes, pd, metric, 1)
                np.testing.assert_array_equal(e.search_keys(probes, metric), keys, err_msg=f"second call {what}")
                tkeys = e.search_topk_keys(probes, M, metric)
                np.testing.assert_array_equal(tkeys, e.search_topk_keys(pd, M, metric).cpu().numpy())
                return keys, rec, tkeys

            def check_none(keys, rec, tkeys):
                for p in BAD_PROBES:
                    assert keys[p] == NONE and rec["key"][p] == NONE, (what, p)
                    assert rec["score"][p] == np.inf and rec["scale"][p] == 0.0, (what, p)
                    assert (tkeys[p] == NONE).all(), (what, p)

            # finite gallery: the finite probes alone, then with the non-finite ones among them
            keys0, rec0, tkeys0 = run(g, q[fin])
            pu.assert_exact_argbest(q[fin], g, _rows(keys0), metric, ref=ref_clean)
            keys1, rec1, tkeys1 = run(g, q_bad, qd_bad)
            np.testing.assert_array_equal(keys1[fin], keys0, err_msg=f"finite probes, finite gallery {what}")
            np.testing.assert_array_equal(_as_int64(rec1[fin]), _as_int64(rec0))
            np.testing.assert_array_equal(tkeys1[fin], tkeys0)
            check_none(keys1, rec1, tkeys1)
            # gallery with non-finite rows against the gallery without them
            keys2, rec2, tkeys2 = run(g[kept], q[fin])
            pu.assert_exact_argbest(q[fin], g[kept], _rows(keys2), metric, ref=ref_kept)
            keys3, rec3, tkeys3 = run(g_bad, q_bad, qd_bad)
            check_none(keys3, rec3, tkeys3)
            rows3 = _rows(keys3)[fin]
            assert not np.isin(rows3, list(BAD_ROWS)).any(), what
            np.testing.assert_array_equal(rows3, kept[_rows(keys2)], err_msg=f"finite probes, bad gallery {what}")
            np.testing.assert_array_equal(rec3["score"][fin], rec2["score"])
            np.testing.assert_array_equal(rec3["scale"][fin], rec2["scale"])
            trows3 = _rows(tkeys3)[fin]
            assert not np.isin(trows3, list(BAD_ROWS)).any(), what
            np.testing.assert_array_equal(trows3, kept[_rows(tkeys2)], err_msg=f"top-m, bad gallery {what}")


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("k", [13, 600])
def test_a_non_finite_row_does_not_beat_a_poor_match(e, k, bad):
    """Three rows: the probes' own direction with one non-finite component, and two rows that
    point the other way (cosine ~ -1, the largest L2 distances).  Any score the non-finite row got
    other than NaN or +inf, such as the 0 a zero vector scores under cosine, would beat both finite
    rows.  The finite rows must come back, in the order of the gallery without row 0; a top-m list
    longer than the finite rows ends in empty slots; the labelled sweep follows the same rule."""
    rng = np.random.default_rng(300 + k)
    q0 = rng.standard_normal(k).astype(np.float32)
    b, n = 5, 3
    q = (q0 * (1 + 0.01 * rng.standard_normal((b, k)))).astype(np.float32)
    g = np.stack([q0, -q0, -q0 + 0.1 * rng.standard_normal(k)]).astype(np.float32)
    g[0, 1] = bad
    kept = g[1:]
    qd = torch.as_tensor(q).cuda()
    glab = np.zeros(n, np.int32)
    plab = np.zeros(b, np.int32)

    def local(rows):  # rows of g -> rows of kept, -1 for an empty slot
        assert (rows != 0).all(), "the non-finite row was returned"
        return np.where(rows < 0, -1, rows - 1)

    e.set_gallery(g, global_offset=OFFSET)
    e.set_gallery_labels(glab)
    for metric in METRICS:
        ref1 = pu.top2(q, kept, metric)
        refm = Reference(q, kept, metric, ranks=M)
        for split in (0, 1):
            what = (k, bad, metric, split)
            e.set_option("search_split_bf16", split)
            keys, rec = _top1(e, q, qd, metric, 1)
            idx = local(_rows(keys))
            assert ((idx >= 0) & (idx < len(kept))).all(), what
            assert pu.assert_exact_argbest(q, kept, idx, metric, ref=ref1).all(), what
            want = _fp64_scores(q, kept, idx, metric)
            assert (np.abs(rec["score"] - want) <= 1e-12 * np.abs(want)).all(), what
            np.testing.assert_array_equal(rec["key"], keys)
            for cand in (1024, 16):
                e.set_option("search_topk_cand", cand)
                tkeys = e.search_topk_keys(q, M, metric)
                np.testing.assert_array_equal(tkeys, e.search_topk_keys(qd, M, metric).cpu().numpy())
                assert check_topk(refm, M, local(_rows(tkeys))).all(), what  # M = 3 slots, 2 finite rows
                assert (tkeys[:, 2] == NONE).all(), what
                np.testing.assert_array_equal(tkeys[:, 0], keys)
            e.set_option("search_topk_cand", 1024)
        # labelled sweep: the same answer; with the winner excluded, the other finite row
        same = e.search_labelled_keys(q, plab, "same", None, metric)
        np.testing.assert_array_equal(same, keys, err_msg=f"labelled {what}")
        rest = e.search_labelled_keys(q, plab, "same", (keys & 0xFFFFFFFF).astype(np.int64), metric)
        np.testing.assert_array_equal(local(_rows(rest)), 1 - idx, err_msg=f"labelled, winner excluded {what}")
        assert (e.search_labelled_keys(q, plab, "other", None, metric) == NONE).all(), what
