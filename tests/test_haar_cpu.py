"""CPU checks of the Haar detector's oracle and host logic: cv::groupRectangles
restatement, the invoker's skip rule, scale list, and the product's cascade-XML loader;
and the input conditions of the GPU edge tests (tests/test_gpu_haar_edges.py)."""
import numpy as np
import pytest

from haar_util import (BRIGHT_FINE, STAGE_COUNTS, THIRD_WINS, bright_case, cascade_xml, directed_walk_rows, long_stage_case,
                       order_free, shared_corners, stage_census, stage_count_case, synth_cascade, synth_frame,
                       third_case, walk_cascade, walk_expected, walk_frame, walk_rows_for_count, wide_case)
from oracle import haar_oracle as ho
from oracle.image_oracle import resize_linear


def test_group_rectangles_rules():
    a = [(10, 10, 30, 30)] * 6 + [(11, 10, 30, 31)]          # one cluster of 7
    b = [(100, 100, 40, 40)] * 3                             # below the neighbour threshold
    inner = [(14, 14, 20, 20)] * 6                           # inside the first (n2 > max(3, n1))
    got = ho.group_rectangles(a + b + inner, 5)
    assert got == [(10, 10, 30, 30)]
    # averaging uses float 1/n and round-half-even
    assert ho.group_rectangles([(0, 0, 10, 10), (1, 1, 11, 11)] * 3, 2) == [(0, 0, 10, 10)]
    assert ho.group_rectangles(a, 0) == a


def test_partition_numbers_classes_by_lowest_member():
    rects = [(0, 0, 10, 10), (200, 200, 10, 10), (1, 0, 10, 10), (200, 201, 10, 10), (500, 0, 10, 10)]
    labels, n = ho.partition(rects, 0.2)
    assert labels == [0, 1, 0, 1, 2] and n == 3


def test_scale_list_matches_min_size_rule():
    sc = ho.scale_list((24, 24), (640, 480), 1.1, (30, 30))
    assert abs(sc[0] - 1.331) < 1e-6 and round(24 * float(sc[0])) >= 30
    assert round(24 * float(sc[-1])) <= 480 and round(24 * float(sc[-1]) * 1.1) > 480


def test_candidates_skip_rule():
    """A stage-0 rejection skips the next x position (CascadeClassifierInvoker)."""
    c = synth_cascade(1)
    f = synth_frame(1, (60, 80))
    res = ho.eval_layer(f, c)
    cand = ho.candidates(f, c, 1.1, (24, 24), (24, 24))  # one scale: factor 1
    exp = []
    for y in range(0, res.shape[0], 2):
        x = 0
        while x < res.shape[1]:
            if res[y, x] > 0:
                exp.append((x, y, 24, 24))
            x += 4 if res[y, x] == 0 else 2
    assert cand == exp
    assert (res == -1).any() and (res == 0).any() and (res == 1).any()


def test_load_cascade_roundtrip(tmp_path):
    from eigenface.haar import load_cascade
    c = synth_cascade(2)
    p = tmp_path / "c.xml"
    p.write_text(cascade_xml(c))
    got = load_cascade(str(p))
    assert got["win"] == c["win"]
    assert [[tuple(r) for r in f] for f in got["features"]] == [[tuple(r) for r in f] for f in c["features"]]
    assert got["stages"] == c["stages"]


# ---------------------------------------------------------------------------------------
# Input conditions of tests/test_gpu_haar_edges.py, stated where no GPU is needed: a GPU
# comparison on an input that never reaches the code in question would pass emptily.

def _census_ok(layer, c):
    lowvar, rej, passed = stage_census(layer, c)
    res = ho.eval_layer(layer, c)
    assert min(rej) > 0, f"a stage rejects nothing that reached it: {rej}"
    assert passed > 0 and lowvar > 0
    assert (res == -1).any() and (res == 0).any() and (res == 1).any()


@pytest.mark.parametrize("bits", [directed_walk_rows(200)[:24], directed_walk_rows(65)[-24:],
                                  np.ones((40, 200), bool), np.zeros((3, 129), bool)],
                         ids=["200", "65", "all_pass_40x200", "all_reject"])
def test_walk_frame_writes_the_bit_matrix(bits):
    """The oracle on walk_frame(bits) is the plain sequential walk over bits (so the stage-0
    results are bits, none is a variance reject, and only the scale-1 layer exists)."""
    c, f = walk_cascade(), walk_frame(bits)
    assert f.shape == (2 * (len(bits) - 1) + 24, 2 * (bits.shape[1] - 1) + 24)
    res = ho.eval_layer(f, c)[::2, ::2]
    assert np.array_equal(res == 1, bits) and np.array_equal(res == 0, ~bits)
    assert ho.candidates(f, c, 1.1, (24, 24), (24, 24)) == walk_expected(bits)
    if bits.all():
        assert len(walk_expected(bits)) == bits.size


def test_directed_walk_rows_cover_the_chunk_edges():
    rows = directed_walk_rows(200)
    rej = ~rows
    runs = set()  # (start, length) of every reject run
    for r in rej:
        e = np.flatnonzero(np.diff(np.r_[0, r.astype(np.int8), 0]))
        runs |= {(int(a), int(b - a)) for a, b in zip(e[::2], e[1::2])}
    for edge in (64, 128):
        for parity in (0, 1):
            across = {n for a, n in runs if a % 2 == parity and a < edge < a + n}
            assert set(range(3, 71)) <= across  # every length, both parities, across each edge
    assert {(63, 1), (64, 1), (63, 2), (61, 70), (199, 1), (0, 200)} <= runs
    assert rows.all(1).any() and len(rows) > 24  # all-pass; several 24-row frames
    for npos in (63, 64, 65, 128, 129):
        assert directed_walk_rows(npos).shape[1] == npos


@pytest.mark.parametrize("nrows", [1, 15, 16, 17])
def test_walk_row_count_selections_are_not_empty(nrows):
    """The rows of the GPU row-count test: the first and the last row emit windows from all
    four chunks and skip in them, every row emits, and a reject run lies across
    position 63/64 — so a row the kernel lost would be missed."""
    bits = walk_rows_for_count(nrows)
    assert bits.shape == (nrows, 200)
    for r in {0, nrows - 1}:
        emitted = {x // 2 // 64 for x, y, _, _ in walk_expected(bits) if y == 2 * r}
        assert emitted == {0, 1, 2, 3}
        assert (~bits[r]).reshape(-1)[:192].reshape(3, 64).any(1).all()
    per_row = np.bincount([y // 2 for _, y, _, _ in walk_expected(bits)], minlength=nrows)
    assert (per_row > 0).all()
    assert any(not row[63] and not row[64] for row in bits)
    f = walk_frame(bits)
    assert ho.candidates(f, walk_cascade(), 1.1, (24, 24), (24, 24)) == walk_expected(bits)


@pytest.mark.parametrize("win", THIRD_WINS)
def test_third_cases_reach_every_stage_and_the_third_rectangle(win):
    c, f = third_case(win)
    _census_ok(f, c)
    assert order_free(c)  # so the split kernel runs unless the ordered form is forced
    used = {fi for _, st in c["stages"] for fi, *_ in st}
    live = [i for i in sorted(used) if len(c["features"][i]) == 3 and c["features"][i][2][4] != 0]
    assert len(live) * 2 >= len(used)
    for i in live:  # OpenCV's features are zero-mean: sum(weight * area) == 0
        assert sum(w * h * wt for _, _, w, h, wt in c["features"][i]) == 0
        assert all(x >= 0 and y >= 0 and x + w <= win[0] and y + h <= win[1] for x, y, w, h, _ in c["features"][i])
    # the third term is observable: without it some stump decides otherwise on this frame,
    # or no window's result could change
    two = dict(c, features=[ft[:2] for ft in c["features"]])
    assert (ho.eval_layer(f, c) != ho.eval_layer(f, two)).any()


def test_third_features_reach_every_corner_sharing_state():
    """Over the cascades of the third-rectangle tests: rectangle 1 shares 0, 1, 2 and 4
    corners with rectangle 0, and each of -1, 0, 1, 2, 3 occurs for rectangle 1 and for
    rectangle 2; the diagonal family and the no-shared-corner family are both present."""
    feats = [ft for win in THIRD_WINS for ft in third_case(win)[0]["features"] if len(ft) == 3 and ft[2][4] != 0]
    tabs = [shared_corners(ft) for ft in feats]
    assert {sum(k >= 0 for k in t[0]) for t in tabs} >= {0, 1, 2, 4}
    for r in (0, 1):
        assert {k for t in tabs for k in t[r]} == {-1, 0, 1, 2, 3}
    assert any(all(k < 0 for k in t[0] + t[1]) for t in tabs)
    diag = [ft for ft in feats if ft[0][4] == -1 and ft[1][4] == ft[2][4] == 2 and ft[1][2] * 2 == ft[0][2]
            and ft[1][3] * 2 == ft[0][3] and abs(ft[1][0] - ft[2][0]) == ft[1][2] and abs(ft[1][1] - ft[2][1]) == ft[1][3]]
    assert diag


def test_third_zero_keeps_every_seed():
    """third=0 (the default) leaves the cascades of the existing tests unchanged, and a
    third share replaces features only."""
    for seed in (0, 1, 7):
        a, b = synth_cascade(seed), synth_cascade(seed, third=0.5)
        assert a["stages"] == b["stages"] and a["features"] != b["features"]
    import hashlib  # digests taken before the `third` argument existed
    for kw, digest in [(dict(seed=0), "5f371f78a67fc4f7"), (dict(seed=3, loose=0.3), "c7913ad9c624fa02"),
                       (dict(seed=8, n_feat=60, stages=tuple(range(3, 43, 2)), loose=2.7), "f6babe429eeef05b")]:
        assert hashlib.sha1(repr(synth_cascade(**kw)).encode()).hexdigest()[:16] == digest


@pytest.mark.parametrize("n", STAGE_COUNTS)
def test_stage_count_cases_reach_every_stage(n):
    c, f = stage_count_case(n)
    assert len(c["stages"]) == n and order_free(c)
    _census_ok(f, c)


def test_long_stage_case_reaches_the_second_record_chunk():
    c, f = long_stage_case()
    assert [len(s) for _, s in c["stages"]] == [3, 300, 5] and order_free(c)
    _census_ok(f, c)  # windows reach the 300-stump stage, are rejected by it and pass it


def test_wide_case_has_step1_rows_of_many_chunks():
    """Rows of the scan walk are cut into chunks of 64 positions: the 640-wide frame gives
    step-1 layers (scale >= 2) with rows of four and five chunks, and step-2 layers of five."""
    c, f = wide_case()
    _census_ok(f, c)
    chunks = {1: [], 2: []}
    for sc in ho.scale_list(c["win"], (640, 80), 1.1):
        step = 1 if sc >= 2 else 2
        res = ho.eval_layer(resize_linear(f, ho.layer_size((640, 80), sc)), c)[::step, ::step]
        if res.shape[1] > 192:
            chunks[step].append(-(-res.shape[1] // 64))
            assert (res == 0).any() and (res == 1).any()  # the walk both skips and emits
    assert len(chunks[1]) >= 3 and max(chunks[1]) == 5 and max(chunks[2]) == 5


def test_bright_case_wraps_the_square_sums():
    """The frame's sum of squares passes 2^32.  At scale factor 1.1 the second layer holds
    1 / 1.21 of it and stays just below, so the GPU test also runs the pyramid of BRIGHT_FINE,
    whose first four layers all pass 2^32 (asserted below; the fifth does not)."""
    c, f = bright_case()
    assert f.shape == (300, 420) and (f.astype(np.int64) ** 2).sum() > 2 ** 32
    sf, mn, mx = BRIGHT_FINE
    scales = ho.scale_list(c["win"], (420, 300), sf, mn, mx)
    assert len(scales) >= 4
    for sc in scales[:4]:
        layer = resize_linear(f, ho.layer_size((420, 300), sc))
        assert (layer.astype(np.int64) ** 2).sum() > 2 ** 32
    _census_ok(f, c)


def test_edge_frames_hold_a_passing_window():
    """The window-sized and one-larger frames of the GPU edge tests hold exactly one
    visitable window and it passes the cascade; the 60 x 200 crop ends its pyramid by
    height while its width would allow more layers."""
    c, f = third_case((24, 24))
    for shape in ((24, 24), (25, 25)):
        assert ho.candidates(f[:shape[0], :shape[1]], c, 1.1, (0, 0)) == [(0, 0, 24, 24)]
    assert ho.candidates(f[:23, :40], c, 1.1, (0, 0)) == [] and ho.candidates(f[:40, :23], c, 1.1, (0, 0)) == []
    assert len(ho.scale_list((24, 24), (200, 60), 1.1)) < len(ho.scale_list((24, 24), (200, 200), 1.1))
    _census_ok(f[20:80, 60:260], c)
