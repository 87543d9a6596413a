"""Top-m search (ef_search_topk) on the GPU against the fp64 numpy checker of
topk_util: distinct rows in fp64 (score, row) order, rank 0 = ef_search's key bit for bit,
first-index ties, EF_KEY_NONE padding, the refinement round and the full-sweep fallback of
overflowing candidate lists, shard merges, device tensors, and the shared workspaces."""
import numpy as np
import pytest

from conftest import golden
from eigenface import Engine, decode_keys, merge_topk_host
from eigenface import _native as N
from parity_util import plant_rivals
from topk_util import Reference, check_topk

pytestmark = pytest.mark.gpu

NONE = N.EF_KEY_NONE
METRICS = ("l2", "cosine")
B = 300  # a ragged second probe tile


@pytest.fixture
def e(eng):
    """The session engine with the search options at their defaults before and after."""
    def reset():
        eng.set_option("search_split_bf16", 0)
        eng.set_option("search_topk_cand", 1024)
    reset()
    yield eng
    reset()


def _rows(keys):
    k = np.asarray(keys)
    return np.where(k == NONE, -1, k & 0xFFFFFFFF)


def _tile_rows(k, split):
    """Gallery rows per scan tile: the chunks of a top-m plan are whole tiles."""
    return 64 if k <= 128 else (256 if split else 128)


# 1. random parity + 2. rank 0 on the same data
@pytest.mark.parametrize("k", [8, 32, 128, 256, 640])
@pytest.mark.parametrize("n", [1, 63, 200, 5003])
def test_random_parity(e, n, k):
    rng = np.random.default_rng(1000 * k + n)
    g = rng.standard_normal((n, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    e.set_gallery(g)
    for metric in METRICS:
        ref = Reference(q, g, metric)
        # the checker alone decides every rank: nothing sits inside a tie window
        assert ref.clear(64).all()
        got = {}
        for opt in (0, 1, 3):
            e.set_option("search_split_bf16", opt)
            top1 = e.search_keys(q, metric)
            for m in (1, 2, 5, 16, 64):
                keys = e.search_topk_keys(q, m, metric)
                stats = e.topk_stats()
                idx, best = decode_keys(keys.reshape(-1), metric)
                clear = check_topk(ref, m, idx.reshape(B, m), best.reshape(B, m))
                assert clear.all()
                np.testing.assert_array_equal(keys[:, 0], top1)  # rank 0 is ef_search, bit for bit
                assert stats[0] == B and stats[2] == 0
                if 2 * -(-n // _tile_rows(k, opt != 0)) >= m:  # enough per-chunk scores for a finite cut
                    assert stats[1] == 0, (opt, m, stats)
                got[opt, m] = keys
        for m in (1, 2, 5, 16, 64):
            np.testing.assert_array_equal(got[3, m], got[1, m])  # the screen counts as the split scan
            np.testing.assert_array_equal(got[1, m], got[0, m])  # (and both equal the fp32 scan's keys)


# 2. rank 0 is ef_search
def test_rank0_on_golden_ties(e):
    t = golden("ties.npz")
    g, q = t["gallery"].astype(np.float32), t["probes"].astype(np.float32)
    e.set_gallery(g)
    top1 = e.search_keys(q, "cosine")
    for m in (1, 3, 8):
        keys = e.search_topk_keys(q, m, "cosine")
        np.testing.assert_array_equal(keys[:, 0], top1)
        np.testing.assert_array_equal(_rows(keys)[:, 0], t["idx"])
        check_topk(Reference(q, g, "cosine"), m, _rows(keys))


@pytest.mark.parametrize("scan", [0, 1])
def test_rank0_on_planted_near_ties(e, scan):
    rng = np.random.default_rng(77)
    n, k, m = 5003, 128, 4
    g0 = rng.standard_normal((n, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    e.set_option("search_split_bf16", scan)
    e.set_gallery(g0)
    anchors = e.search(q, "l2")[0]
    g, rivals = plant_rivals(g0, q, anchors, seed=5)
    e.set_gallery(g)
    top1 = e.search_keys(q, "l2")
    keys = e.search_topk_keys(q, m, "l2")
    np.testing.assert_array_equal(keys[:, 0], top1)
    rows = _rows(keys)
    ref = Reference(q, g, "l2")
    check_topk(ref, m, rows)
    # the best two rows are a planted pair: far inside the scan's rounding, outside the tie
    # window, and returned in fp64 order
    s = ref.chosen(rows[:, :2])
    assert (s[:, 0] <= s[:, 1]).all()
    assert (s[:, 1] - s[:, 0] <= 1e-6 * ref.scale).mean() > 0.9
    assert ref.clear(2).all()
    np.testing.assert_array_equal(rows[:, :2], ref.rows[:, :2])
    assert np.isin(rivals, rows[:, :3]).mean() > 0.9


# 3. short and empty galleries
def test_short_and_empty(e):
    rng = np.random.default_rng(3)
    g = rng.standard_normal((3, 20)).astype(np.float32)
    q = rng.standard_normal((40, 20)).astype(np.float32)
    for metric in METRICS:
        e.set_gallery(g)
        idx, best = e.search_topk(q, 5, metric)
        check_topk(Reference(q, g, metric), 5, idx, best)
        assert (idx[:, 3:] == -1).all() and np.isnan(best[:, 3:]).all() and (idx[:, :3] >= 0).all()
        rec = e.search_topk_matches(q, 5, metric)
        check_topk(Reference(q, g, metric), 5, idx, records=rec)
        e.set_gallery(g[:0])
        keys = e.search_topk_keys(q, 5, metric)
        assert keys.shape == (40, 5) and (keys == NONE).all()
        rec = e.search_topk_matches(q, 5, metric)
        assert (rec["key"] == NONE).all() and np.isinf(rec["score"]).all() and (rec["scale"] == 0).all()
        assert e.topk_stats()[:3] == (40, 0, 0)


# 4. duplicates come out in ascending index
def test_duplicates_ascend(e):
    rng = np.random.default_rng(4)
    g = rng.standard_normal((1000, 64)).astype(np.float32)
    where = np.sort(rng.choice(np.arange(6, 1000), 40, replace=False))
    g[where] = g[5]
    q = np.repeat(g[5:6], 7, axis=0)
    e.set_gallery(g)
    want = np.concatenate([[5], where])[:10]
    for metric in METRICS:
        rows = _rows(e.search_topk_keys(q, 10, metric))
        np.testing.assert_array_equal(rows, np.tile(want, (7, 1)))


def _cluster_case():
    rng = np.random.default_rng(5)
    n, k = 5003, 32
    c = rng.standard_normal(k)
    g = (rng.standard_normal((n, k)) + 10.0).astype(np.float32)
    g[:64] = (c + 0.01 * rng.standard_normal((64, k))).astype(np.float32)  # one tile: one chunk under any plan
    q = (c + 0.01 * rng.standard_normal((B, k))).astype(np.float32)
    return g, q


# 5. the refinement round
def test_refinement_round(e):
    g, q = _cluster_case()
    e.set_gallery(g)
    e.set_option("search_topk_cand", 16)
    for metric in METRICS:
        ref = Reference(q, g, metric)
        keys = e.search_topk_keys(q, 4, metric)
        stats = e.topk_stats()
        # tau is the best score of another chunk, so each first list holds the whole 64-row cluster
        assert stats[0] == B and stats[1] == B, stats
        idx, best = decode_keys(keys.reshape(-1), metric)
        check_topk(ref, 4, idx.reshape(B, 4), best.reshape(B, 4))
        e.set_option("search_topk_cand", 1024)
        np.testing.assert_array_equal(e.search_topk_keys(q, 4, metric), keys)  # results do not depend on it
        assert e.topk_stats()[1] == 0
        e.set_option("search_topk_cand", 16)


# 6. the full-sweep fallback
def test_full_sweep_fallback(e):
    rng = np.random.default_rng(6)
    row = rng.standard_normal(32).astype(np.float32)
    g = np.tile(row, (3000, 1))
    q = rng.standard_normal((8, 32)).astype(np.float32)
    e.set_gallery(g)
    e.set_option("search_topk_cand", 16)
    for metric in METRICS:
        rec = e.search_topk_matches(q, 5, metric)
        stats = e.topk_stats()
        np.testing.assert_array_equal(rec["key"] & 0xFFFFFFFF, np.tile(np.arange(5), (8, 1)))
        assert stats[1] == 8 and stats[2] == 8, stats
        check_topk(Reference(q, g, metric), 5, _rows(rec["key"]), records=rec)
        np.testing.assert_array_equal(e.search_topk_keys(q, 1, metric)[:, 0], e.search_keys(q, metric))


def test_argument_checks(e):
    from eigenface import EigenfaceError
    g = np.zeros((10, 8), np.float32)
    e.set_gallery(g)
    with pytest.raises(ValueError):
        e.search_topk_keys(g, 0)
    with pytest.raises(ValueError):
        e.search_topk_keys(g, 65)
    keys = np.empty((10, 65), np.int64)
    lib = N.lib()
    for m in (0, 65):
        assert lib.ef_search_topk(e._h, g.ctypes.data, 10, m, 0, keys.ctypes.data, 0) == -1  # EF_E_INVALID
    e.set_option("search_topk_cand", 16)
    with pytest.raises(EigenfaceError):
        e.search_topk_keys(g, 17)
    for bad in (15, 4097):
        with pytest.raises(EigenfaceError):
            e.set_option("search_topk_cand", bad)
    assert e.get_option("search_topk_cand") == 16


# 7. shards
def test_shards_merge_to_the_single_engine_answer(e):
    import torch
    rng = np.random.default_rng(7)
    n, k, cut = 5003, 48, 2500
    g = rng.standard_normal((n, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    qd = torch.from_numpy(q).cuda()
    with Engine(0) as e2:
        e.set_gallery(g)
        want = {(m, mt): e.search_topk_keys(q, m, mt) for m in (1, 10) for mt in METRICS}
        e.set_gallery(g[:cut], global_offset=0)
        e2.set_gallery(g[cut:], global_offset=cut)
        for (m, mt), full in want.items():
            parts = torch.stack([e.search_topk_matches(qd, m, mt), e2.search_topk_matches(qd, m, mt)])
            assert parts.shape == (2, B, m, 3)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(e.merge_topk(parts, B, m).cpu().numpy(), full)
            np.testing.assert_array_equal(merge_topk_host(parts.cpu().numpy(), B, m), full)
            host = np.stack([e.search_topk_matches(q, m, mt), e2.search_topk_matches(q, m, mt)])
            np.testing.assert_array_equal(merge_topk_host(host, B, m), full)


# 8. device tensors on the torch stream
def test_device_tensors_equal_host_call(e):
    import torch
    rng = np.random.default_rng(8)
    g = rng.standard_normal((5003, 100)).astype(np.float32)
    q = rng.standard_normal((B, 100)).astype(np.float32)
    e.set_gallery(g)
    host = e.search_topk_keys(q, 7, "l2")
    qd = torch.from_numpy(q).cuda()
    dev = e.search_topk_keys(qd, 7, "l2")
    assert dev.is_cuda and dev.shape == (B, 7)
    np.testing.assert_array_equal(dev.cpu().numpy(), host)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        out = torch.empty((B, 7), dtype=torch.int64, device="cuda")
        assert e.search_topk_keys(qd * 1.0, 7, "l2", keys=out) is out
        np.testing.assert_array_equal(out.cpu().numpy(), host)
    finally:
        e.use_own_stream()
    idx, best = e.search_topk(qd, 7, "l2")
    np.testing.assert_array_equal(idx, _rows(host))


# 9. the shared workspaces leave the top-1 search as it was
@pytest.mark.parametrize("k", [128, 512])
def test_top1_search_unchanged_after_topk(e, k):
    rng = np.random.default_rng(9 + k)
    g = rng.standard_normal((5003, k)).astype(np.float32)
    q = rng.standard_normal((B, k)).astype(np.float32)
    e.set_gallery(g)
    for opt in (0, 1, 3):
        e.set_option("search_split_bf16", opt)
        for metric in METRICS:
            before = e.search_keys(q, metric)
            rec_before = e.search_matches(q, metric)
            e.search_topk_keys(q, 64, metric)
            e.search_topk_matches(q, 3, metric)
            np.testing.assert_array_equal(e.search_keys(q, metric), before)
            np.testing.assert_array_equal(e.search_matches(q, metric), rec_before)


def test_recognize_topk_and_wrappers(e):
    from eigenface import EigenfacePCA, recognize_face_candidates_with_model, recognize_face_with_model
    from oracle import eigenface_oracle as orc
    x, _ = orc.synth_faces(120, 16, r=12, seed=2)
    mdl = EigenfacePCA(12, standardize=False).fit(x)
    idx, best = mdl.recognize_topk(x[:50], 5, "cosine")
    i1, b1 = mdl.recognize(x[:50], "cosine")
    np.testing.assert_array_equal(idx[:, 0], i1)
    np.testing.assert_array_equal(best[:, 0], b1)
    import torch
    from eigenface import get_engine
    dev_keys = get_engine(0).recognize_topk_keys(torch.from_numpy(x[:50]).cuda(), 5, "cosine")
    np.testing.assert_array_equal(_rows(dev_keys.cpu().numpy()), idx)
    feats = mdl.transform(x[:50]).astype(np.float32)
    check_topk(Reference(feats, mdl.face_features_.astype(np.float32), "cosine"), 5, idx)
    thr = mdl.recognize_topk(x[:50], 5, "cosine", threshold=0.99)[0]
    assert ((thr == -1) == (best < 0.99)).all()
    data = {"face_features": mdl.face_features_, "face_labels": np.arange(120) // 4,
            "person_id_map": {f"p{i}": i for i in range(30)}}
    cands = recognize_face_candidates_with_model(feats[7], data, top=5)
    assert len(cands) == 5 and cands[0] == recognize_face_with_model(feats[7], data, threshold=-2.0)
    assert [c[0] for c in cands] == [int(i) // 4 for i in idx[7]]
    assert [c[1] for c in cands] == [f"p{int(i) // 4}" for i in idx[7]]
    assert all(cands[j][2] >= cands[j + 1][2] for j in range(1, 4))
