"""GPU Haar detector against oracle/haar_oracle.py, exactly, on the inputs the first suite
(test_gpu_haar.py) never gives it: live third rectangles, other window sizes, directed
scan-walk patterns across the 64-position chunks, stage counts at the stage-group
boundaries, a stage longer than one LDS record chunk, the ordered and the split kernel on
the same input, square sums past 2^32, size gates, frame edge sizes, strided and
device-resident frames, host-side argument errors and the wrapper's capacity retry.
tests/test_haar_cpu.py asserts that each input reaches the code it is meant for."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from haar_util import (BRIGHT_FINE, STAGE_COUNTS, THIRD_WINS, bright_case, directed_walk_rows, long_stage_case,
                       stage_count_case, synth_cascade, synth_frame, third_case, walk_cascade, walk_expected,
                       walk_frame, walk_rows_for_count, wide_case)
from oracle import haar_oracle as ho

pytestmark = pytest.mark.gpu

_REF = {}
EF_E_INVALID = -1  # include/eigenface.h


def _ref(key, f, c, sf=1.1, mn=(0, 0), mx=None):
    """The oracle's candidates, computed once per input (several tests share them)."""
    if key not in _REF:
        _REF[key] = ho.candidates(f, c, sf, mn, mx)
    return _REF[key]


@contextmanager
def _classifier(c, ordered=0):
    """The option is read when the cascade is set: set it first, restore it afterwards."""
    from eigenface.haar import CascadeClassifier
    from eigenface.pca import get_engine
    e = get_engine(0)
    old = e.get_option("haar_ordered")
    e.set_option("haar_ordered", ordered)
    try:
        yield CascadeClassifier(cascade=c, engine=e)
    finally:
        e.set_option("haar_ordered", old)


def _check(clf, f, ref, sf=1.1, mn=(0, 0), mx=(), mns=2):
    """Candidates in order; grouped rectangles too where the oracle's quadratic grouping is
    affordable, else minNeighbors = 0, which must hand the candidates through."""
    if len(ref) > 2000:
        mns = 0
    rects, cand = clf.detect(f, sf, mns, mn, mx, return_candidates=True)
    assert [tuple(r) for r in cand] == ref
    assert [tuple(r) for r in rects] == ho.group_rectangles(ref, mns)


# ------------------------------------------------ 1, 6: third rectangle, window sizes, both forms
@pytest.mark.parametrize("ordered", [0, 1])
@pytest.mark.parametrize("sf", [1.1, 1.25])
@pytest.mark.parametrize("win", THIRD_WINS, ids=lambda w: f"{w[0]}x{w[1]}")
def test_third_rectangle_and_window_sizes(win, sf, ordered):
    c, f = third_case(win)
    ref = _ref(("third", win, sf), f, c, sf)
    assert len(ref) > 0
    with _classifier(c, ordered) as clf:
        _check(clf, f, ref, sf)


@pytest.mark.parametrize("ordered", [0, 1])
@pytest.mark.parametrize("nst,shape,seed", [(12, (120, 160), 7), (20, (150, 200), 8)])
def test_long_cascades_ordered_equals_split(nst, shape, seed, ordered):
    """The cascades of test_long_cascade_split_and_ordered_paths with the ordered form forced
    by the option (not by a leaf value) and with the split form: both equal the oracle."""
    c = synth_cascade(seed, n_feat=60, stages=tuple(range(3, 3 + 2 * nst, 2)), loose=2.0 if nst <= 12 else 2.7)
    f = synth_frame(3, shape)
    ref = _ref(("long", nst), f, c)
    assert len(ref) > 0
    with _classifier(c, ordered) as clf:
        _check(clf, f, ref)


# ------------------------------------------------ 2: directed scan walk
def _walk_frames(rows, per=24):
    for i in range(0, len(rows), per):
        yield rows[i:i + per]


@pytest.mark.parametrize("npos", [200, 63, 64, 65, 128, 129])
def test_directed_walk(npos):
    """Every directed row (haar_util.directed_walk_rows), 24 evaluated rows per frame: the
    candidates are the sequential walk over the intended bits, which the oracle confirms."""
    c = walk_cascade()
    with _classifier(c) as clf:
        for bits in _walk_frames(directed_walk_rows(npos)):
            f = walk_frame(bits)
            _, cand = clf.detect(f, 1.1, 0, (24, 24), (24, 24), return_candidates=True)
            exp = walk_expected(bits)
            assert [tuple(r) for r in cand] == exp
            assert ho.candidates(f, c, 1.1, (24, 24), (24, 24)) == exp


@pytest.mark.parametrize("nrows", [1, 15, 16, 17])
def test_directed_walk_row_counts(nrows):
    """One workgroup of the walk kernel covers 16 rows: one row, one short of a workgroup,
    exactly one, and one more."""
    bits = walk_rows_for_count(nrows)
    c, f = walk_cascade(), walk_frame(bits)
    with _classifier(c) as clf:
        _, cand = clf.detect(f, 1.1, 0, (24, 24), (24, 24), return_candidates=True)
    assert [tuple(r) for r in cand] == walk_expected(bits) == ho.candidates(f, c, 1.1, (24, 24), (24, 24))


# ------------------------------------------------ 3: wide step-1 layers
def test_wide_step1_layers():
    c, f = wide_case()
    ref = _ref("wide", f, c)
    assert len(ref) > 0
    with _classifier(c) as clf:
        _check(clf, f, ref)


# ------------------------------------------------ 4: stage counts at the group boundaries
@pytest.mark.parametrize("n", STAGE_COUNTS)
def test_stage_count_boundaries(n):
    """Stage groups start at stages 1, 4, 8 and 14: cascades ending on a group's last stage
    or one past it, and the one-stage cascade, which launches no group and returns stage 0's
    survivors."""
    c, f = stage_count_case(n)
    ref = _ref(("stages", n), f, c)
    assert len(ref) > 0
    with _classifier(c) as clf:
        _check(clf, f, ref)


# ------------------------------------------------ 5: a stage longer than one record chunk
@pytest.mark.parametrize("ordered", [0, 1])
def test_long_stage(ordered):
    c, f = long_stage_case()
    ref = _ref("long_stage", f, c)
    assert len(ref) > 0
    with _classifier(c, ordered) as clf:
        _check(clf, f, ref)


# ------------------------------------------------ 7: sums of squares past 2^32
@pytest.mark.parametrize("sf,mn,mx", [(1.1, (0, 0), ()), BRIGHT_FINE], ids=["sf1.1", "sf1.03_max27"])
def test_square_sums_wrap(sf, mn, mx):
    """uint32 integral of squares against the oracle's int64 (candidates only; the plain
    int32 sum would need a frame of more than 8.4 Mpx to wrap, which no test here has)."""
    c, f = bright_case()
    ref = _ref(("bright", sf), f, c, sf, mn, mx or None)
    assert len(ref) > 4096
    with _classifier(c) as clf:
        _, cand = clf.detect(f, sf, 0, mn, mx, return_candidates=True)
    assert [tuple(r) for r in cand] == ref


# ------------------------------------------------ 8: size gates
@pytest.mark.parametrize("mn,mx", [((0, 0), (48, 48)), ((0, 0), (60, 40)), ((24, 24), (24, 24)), ((47, 47), (47, 47)),
                                   ((51, 51), (51, 51)), ((40, 24), ()), ((30, 40), (70, 90))])
def test_size_gates(mn, mx):
    """maxSize, minSize = maxSize (a single layer: the first, a step-2 one at scale 1.95, a
    step-1 one at 2.14) and non-square sizes."""
    c, f = third_case((24, 24))
    ref = _ref(("gates", mn, mx), f, c, 1.1, mn, mx or None)
    assert len(ref) > 0
    if mn == mx:
        assert len({r[2:] for r in ref}) == 1 and ref[0][2:] == mn
    with _classifier(c) as clf:
        _check(clf, f, ref, 1.1, mn, mx)


def test_min_neighbors_zero_returns_candidates():
    c, f = third_case((24, 24))
    ref = _ref(("gates", (47, 47), (47, 47)), f, c, 1.1, (47, 47), (47, 47))
    with _classifier(c) as clf:
        rects, cand = clf.detect(f, 1.1, 0, (47, 47), (47, 47), return_candidates=True)
        grouped, _ = clf.detect(f, 1.1, 2, (47, 47), (47, 47), return_candidates=True)
    assert [tuple(r) for r in rects] == [tuple(r) for r in cand] == ref
    assert [tuple(r) for r in grouped] == ho.group_rectangles(ref, 2) != ref


# ------------------------------------------------ 9: frame edge sizes
def test_frame_edge_sizes():
    c, f = third_case((24, 24))
    with _classifier(c) as clf:
        for shape in ((24, 24), (25, 25)):  # one window, which passes (test_haar_cpu.py)
            rects, cand = clf.detect(f[:shape[0], :shape[1]], 1.1, 0, return_candidates=True)
            assert [tuple(r) for r in cand] == [tuple(r) for r in rects] == [(0, 0, 24, 24)]
        for g in (f[:23, :40], f[:40, :23]):  # smaller than the window: nothing, no error
            rects, cand = clf.detect(g, 1.1, 0, return_candidates=True)
            assert len(rects) == 0 and len(cand) == 0
            assert clf.detectMultiScale(g) == ()
        g = f[20:80, 60:260]  # the pyramid ends by height while the width allows more layers
        _check(clf, g, _ref("h60", g, c))


# ------------------------------------------------ 10: memory forms through the C entry point
def _raw_detect(e, ptr, H, W, ld, flags, sf=1.1, mns=2, cap=1 << 16):
    out, cand = np.empty((cap, 4), np.int32), np.empty((cap, 4), np.int32)
    n, nc = C.c_int32(0), C.c_int32(0)
    e._chk(e._lib.ef_haar_detect(e._h, ptr, H, W, ld, sf, mns, 0, 0, 0, 0, out.ctypes.data, cap, C.byref(n),
                                 cand.ctypes.data, cap, C.byref(nc), flags))
    assert n.value <= cap and nc.value <= cap
    return [tuple(r) for r in out[:n.value]], [tuple(r) for r in cand[:nc.value]]


def test_strided_and_device_frames():
    """Host rows with ld = W + 13, a device-resident frame, and a device frame with
    ld > W give what the contiguous host frame gives (and the oracle)."""
    import torch
    from eigenface import _native as N
    c, f = third_case((24, 24))
    f = np.ascontiguousarray(f[20:80, 60:260])
    H, W = f.shape
    ref = _ref("h60", f, c)
    mns = 2 if len(ref) <= 2000 else 0
    want = (ho.group_rectangles(ref, mns), ref)
    wide = np.full((H, W + 13), 255, np.uint8)  # sentinel in the padding
    wide[:, :W] = f
    with _classifier(c) as clf:
        e = clf.engine
        assert _raw_detect(e, f.ctypes.data, H, W, W, 0, mns=mns) == want
        assert _raw_detect(e, wide.ctypes.data, H, W, W + 13, 0, mns=mns) == want
        assert (wide[:, W:] == 255).all()
        d = torch.from_numpy(f).cuda()
        dw = torch.from_numpy(wide).cuda()
        torch.cuda.synchronize()  # the uploads ran on torch's stream, the detector has its own
        assert _raw_detect(e, d.data_ptr(), H, W, W, N.EF_MEM_DEVICE, mns=mns) == want
        assert dw.stride(0) == W + 13
        assert _raw_detect(e, dw.data_ptr(), H, W, W + 13, N.EF_MEM_DEVICE, mns=mns) == want
        assert torch.equal(dw.cpu(), torch.from_numpy(wide))


# ------------------------------------------------ 11: argument errors, reported by the host
def test_argument_errors_are_reported():
    from eigenface import _native as N
    c, f = third_case((24, 24))
    g = f[:60, :200]
    with _classifier(c) as clf:
        before = clf.detect(g, 1.1, 2, return_candidates=True)
        with pytest.raises(N.EigenfaceError, match="pyramid layers") as ei:
            clf.detect(np.ascontiguousarray(f[:100, :200].repeat(2, 0)), 1.0005)  # 200 x 200: > 255 layers
        assert ei.value.code == EF_E_INVALID
        for sf in (1.0, 0.9):
            with pytest.raises(N.EigenfaceError) as ei:
                clf.detect(g, sf)
            assert ei.value.code == EF_E_INVALID
        for bad in ((20, 0, 5, 4, 2.0), (0, 21, 4, 4, 2.0), (-1, 0, 4, 4, 2.0)):  # outside the 24 x 24 window
            broken = dict(c, features=[[c["features"][0][0], bad]] + c["features"][1:])
            with pytest.raises(N.EigenfaceError, match="outside the window") as ei:
                clf.set_cascade(broken)
            assert ei.value.code == EF_E_INVALID
        after = clf.detect(g, 1.1, 2, return_candidates=True)  # the earlier cascade still serves
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert [tuple(r) for r in after[1]] == ho.candidates(g, c, 1.1, (0, 0))


# ------------------------------------------------ 12: the wrapper's capacity retry
def test_capacity_retry():
    """More candidates than the wrapper's first buffer of 4096 holds: 40 rows x 200
    positions, all passing."""
    bits = np.ones((40, 200), bool)
    c, f = walk_cascade(), walk_frame(bits)
    with _classifier(c) as clf:
        rects, cand = clf.detect(f, 1.1, 0, (24, 24), (24, 24), return_candidates=True)
    assert len(cand) == 8000 > 4096
    assert [tuple(r) for r in cand] == ho.candidates(f, c, 1.1, (24, 24), (24, 24)) == walk_expected(bits)
    assert np.array_equal(rects, cand)
