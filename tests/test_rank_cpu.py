"""Identification rank, the parts that need no GPU: the host-only planner against hand-computed
cases, cmc_curve / mean_reciprocal_rank / summarize_identification on a hand-written ``better``,
the symbols, and the numpy reference against a plain loop."""
import ctypes
import os
import re

import numpy as np
import pytest

import rank_util as rk
from eigenface import _native as N
from eigenface import evaluate as ev

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------------ the planner
def _plan(b, n, c, budget):
    w, p, m = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = N.lib().ef_search_rank_plan(b, n, c, budget, ctypes.byref(w), ctypes.byref(p), ctypes.byref(m))
    return rc, w.value, p.value, m.value


@pytest.mark.parametrize("c,words", ((1, 1), (32, 1), (33, 2), (64, 2), (65, 3), (125000, 3907)))
def test_plan_words_per_probe(c, words):
    assert _plan(10, 100, c, 256 << 20) == (N.EF_OK, words, 256, 1)


def test_plan_pieces():
    """b = 1024 probes, C = 33: two words per probe, so a 256-probe block needs 2048 bytes."""
    assert _plan(1024, 1000, 33, 8192) == (N.EF_OK, 2, 1024, 1)     # everything fits: one piece
    assert _plan(1024, 1000, 33, 1 << 40) == (N.EF_OK, 2, 1024, 1)  # never more than the padded probes
    assert _plan(1024, 1000, 33, 4096) == (N.EF_OK, 2, 512, 2)
    assert _plan(1024, 1000, 33, 6143) == (N.EF_OK, 2, 512, 2)      # whole blocks only
    assert _plan(1024, 1000, 33, 6144) == (N.EF_OK, 2, 768, 2)      # 768 + 256
    assert _plan(1024, 1000, 33, 2048) == (N.EF_OK, 2, 256, 4)      # b / 256 pieces
    assert _plan(1024, 1000, 33, 1) == (N.EF_OK, 2, 256, 4)         # below one block's need: one block
    assert _plan(1024, 1000, 33, 0) == (N.EF_OK, 2, 256, 4)
    assert _plan(1000, 1000, 33, 2048) == (N.EF_OK, 2, 256, 4)      # b pads to 1024
    assert _plan(1025, 1000, 33, 2048) == (N.EF_OK, 2, 256, 5)
    assert _plan(300, 1000, 32, 1024) == (N.EF_OK, 1, 256, 2)
    assert _plan(600, 1000, 32, 1024) == (N.EF_OK, 1, 256, 3)
    assert _plan(0, 1000, 33, 4096) == (N.EF_OK, 2, 256, 0)         # no probes, no pieces
    assert _plan(1024, 0, 0, 4096) == (N.EF_OK, 1, 1024, 0)         # an empty gallery: none either
    assert ev.search_rank_plan(1024, 1000, 33, 4096) == (2, 512, 2)
    assert ev.search_rank_plan(4096, 10 ** 6, 125000) == (3907, 4096, 1)  # 64 MB inside the default budget


def test_plan_rejects_bad_arguments():
    for args in ((-1, 10, 3, 4096), (10, -1, 3, 4096), (10, 10, -1, 4096), (10, 10, 3, -1)):
        assert _plan(*args)[0] == N.EF_E_INVALID
        with pytest.raises(N.EigenfaceError):
            ev.search_rank_plan(*args)
    w = ctypes.c_int64(0)
    lib = N.lib()
    assert lib.ef_search_rank_plan(1, 1, 1, 1, None, ctypes.byref(w), ctypes.byref(w)) == N.EF_E_INVALID
    assert lib.ef_search_rank_plan(1, 1, 1, 1, ctypes.byref(w), None, ctypes.byref(w)) == N.EF_E_INVALID
    assert lib.ef_search_rank_plan(1, 1, 1, 1, ctypes.byref(w), ctypes.byref(w), None) == N.EF_E_INVALID


# ------------------------------------------------------------------ host arithmetic on better
BETTER = np.array([0, 0, 2, -1, 4, 9, -1], np.int32)  # ranks 1, 1, 3, 5, 10 of five probes; two have none


def test_cmc_curve():
    r, c = ev.cmc_curve(BETTER)
    np.testing.assert_array_equal(r, np.arange(1, 11))
    np.testing.assert_array_equal(c, [0.4, 0.4, 0.6, 0.6, 0.8, 0.8, 0.8, 0.8, 0.8, 1.0])
    r, c = ev.cmc_curve(BETTER, max_rank=3)
    np.testing.assert_array_equal(r, [1, 2, 3])
    np.testing.assert_array_equal(c, [0.4, 0.4, 0.6])
    r, c = ev.cmc_curve(BETTER, max_rank=12)
    assert r.size == 12 and c[-1] == 1.0 and c[9] == 1.0 and c[8] == 0.8
    r, c = ev.cmc_curve(np.array([-1, -1]))
    assert r.tolist() == [1] and np.isnan(c).all()
    r, c = ev.cmc_curve(np.zeros(0, np.int32), max_rank=4)
    assert r.size == 4 and np.isnan(c).all()
    r, c = ev.cmc_curve([0, 0, 0])
    assert r.tolist() == [1] and c.tolist() == [1.0]
    for bad in (np.array([0.5]), np.array([[0]]), np.array([-2])):
        with pytest.raises(ValueError):
            ev.cmc_curve(bad)
    with pytest.raises(ValueError):
        ev.cmc_curve(BETTER, max_rank=0)


def test_mean_reciprocal_rank():
    assert ev.mean_reciprocal_rank(BETTER) == pytest.approx((1 + 1 + 1 / 3 + 1 / 5 + 1 / 10) / 5, rel=1e-15)
    assert np.isnan(ev.mean_reciprocal_rank(np.array([-1])))
    assert ev.mean_reciprocal_rank([0, 0]) == 1.0


def test_summarize_identification():
    s = ev.summarize_identification(BETTER)
    assert s["n"] == 7 and s["n_genuine"] == 5 and s["max_rank"] == 10 and s["median_rank"] == 3.0
    assert s["rank"] == {1: 0.4, 5: 0.8, 10: 1.0, 20: 1.0}
    assert s["mrr"] == ev.mean_reciprocal_rank(BETTER)
    assert ev.summarize_identification(BETTER, ranks=(3,))["rank"] == {3: 0.6}
    e = ev.summarize_identification(np.array([-1, -1]))
    assert e["n"] == 2 and e["n_genuine"] == 0 and e["max_rank"] is None
    assert np.isnan(e["rank"][1]) and np.isnan(e["mrr"]) and np.isnan(e["median_rank"])
    with pytest.raises(ValueError):
        ev.summarize_identification(BETTER, ranks=(0,))


# ------------------------------------------------------------------ symbols and prototypes
def test_symbols_and_prototypes():
    lib = N.lib()
    for name in ("ef_search_rank", "ef_search_rank_plan"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name)
    vp, i32, i64, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32
    assert N._SIGS["ef_search_rank"] == ([vp, vp, i64, i32, vp, vp, vp, vp, vp, u32], ctypes.c_int)
    p64 = ctypes.POINTER(i64)
    assert N._SIGS["ef_search_rank_plan"] == ([i64, i64, i64, i64, p64, p64, p64], ctypes.c_int)
    with open(os.path.join(ROOT, "include", "eigenface.h")) as f:
        hdr = f.read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))
    assert ("int ef_search_rank(ef_ctx* ctx, const float* Q, int64_t b, int32_t metric, const int32_t* probe_labels , "
            "const int64_t* exclude_rows , ef_match* genuine , int32_t* better , int64_t* info , "
            "uint32_t flags);") in flat
    assert ("int ef_search_rank_plan(int64_t b, int64_t n, int64_t n_classes, int64_t bitmap_bytes, "
            "int64_t* words_per_probe, int64_t* probes_per_piece, int64_t* n_pieces);") in flat
    assert "#define EF_API_VERSION 7" in hdr
    assert re.search(r"#define EF_KERNEL_RANK 14\b", hdr) and N.EF_KERNEL_RANK == 14
    assert re.search(r"#define EF_OPT_RANK_BITMAP_BYTES 15\b", hdr) and N.EF_OPT_RANK_BITMAP_BYTES == 15
    assert re.search(r"#define EF_RANK_GENUINE_GIVEN 0x1000u", hdr) and N.EF_RANK_GENUINE_GIVEN == 0x1000
    others = [int(v, 16) for v in re.findall(r"#define EF_(?!RANK_GENUINE)\w+ (0x[0-9a-fA-F]+)u", hdr)]
    assert others and all(v & 0x1000 == 0 for v in others)  # a flag bit of its own
    import eigenface
    for name in ("cmc_curve", "mean_reciprocal_rank", "identification_ranks", "summarize_identification",
                 "search_rank_plan"):
        assert hasattr(eigenface, name) and name in eigenface.__all__
    for name in ("search_rank", "recognize_rank"):
        assert hasattr(eigenface.Engine, name)


# ------------------------------------------------------------------ the reference itself
def _plain(q, g, labels, plabels, metric, exclude, offset):
    q64, g64 = np.asarray(q, np.float64), np.asarray(g, np.float64)

    def score(p, r):
        with np.errstate(all="ignore"):
            if metric == "l2":
                return float(((q64[p] - g64[r]) ** 2).sum())
            qq, gg = float((q64[p] ** 2).sum()), float((g64[r] ** 2).sum())
            if not (np.isfinite(qq) and np.isfinite(gg)):
                return float("nan")
            if qq == 0.0 or gg == 0.0:
                return 0.0
            return -float((q64[p] * g64[r]).sum()) / (np.sqrt(qq) * np.sqrt(gg))
    out = []
    for p in range(q64.shape[0]):
        rows = [r for r in range(g64.shape[0]) if r + offset != exclude[p] and np.isfinite(score(p, r))]
        same = [r for r in rows if labels[r] == plabels[p]]
        if not same:
            out.append(-1)
            continue
        gen = min(same, key=lambda r: (score(p, r), r))
        tau = score(p, gen)
        out.append(len({labels[r] for r in rows if labels[r] != plabels[p]
                        and (score(p, r) < tau or (score(p, r) == tau and r < gen))}))
    return np.array(out, np.int32)


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_reference_against_a_plain_loop(metric):
    g, lab, _, names = rk.blobs(150, 9, 11, 5)
    g = g.copy()
    rng = np.random.default_rng(6)
    pick = rng.integers(0, 150, 40)
    q = (g[pick] + 0.5 * rng.standard_normal((40, 9))).astype(np.float32)
    pl = lab[pick].copy()
    g[17] = 0.0
    g[40, 2] = np.nan
    g[60] = g[3]  # a duplicate across identities: the first-index rule decides
    q[5] = 0.0
    q[9, 0] = np.inf
    q[11] = g[3]
    pl[11] = lab[60]
    pl[13] = 2 ** 30  # a label no row carries
    excl = np.full(40, -1, np.int64)
    excl[:12] = pick[:12] + 1000
    excl[3], excl[4] = 999, 1150
    ref = rk.reference(q, g, lab, pl, metric, excl, offset=1000)
    want = _plain(q, g, lab, pl, metric, excl, 1000)
    np.testing.assert_array_equal(ref["better"], want)
    assert ref["better"][9] == -1 and ref["better"][13] == -1 and ref["row_gen"][13] == -1
    assert ref["better"][11] == 1 and ref["row_gen"][11] == 1060  # row 3 ties at a lower index
    assert np.unique(ref["better"]).size >= 4 and (ref["better"] == 0).any()
    fast = rk.better_blocked(q, g, lab, pl, metric, excl, offset=1000, block=7)
    np.testing.assert_array_equal(fast[0], ref["better"])
    np.testing.assert_array_equal(fast[1], ref["row_gen"])
    assert fast[2].any() and not fast[2][[17 if metric == "l2" else 40, 40]].all()
    d = rk.delta(q, g, metric, ref["tau"])
    ok = ref["better"] >= 0
    assert (d[ok] > 0).all() and np.isfinite(d[ok]).all()
