"""ROI ingest (ef_preprocess_rois): rows bit-equal to the oracle's preprocess of the contiguous
crop and to ef_preprocess of the copies — rectangles read in place from a row-strided frame."""
import numpy as np
import pytest

from oracle import image_oracle as io

pytestmark = pytest.mark.gpu

H, W = 97, 131
# x, y, w, h.  Interior rectangles (a clamp to the frame instead of the rectangle would read
# the neighbours outside them), rectangles on the last row / column, the identity (64 x 64),
# 1 x 1 and the two thin shapes.
RECTS = np.array([
    (10, 12, 30, 40), (40, 20, 55, 33), (5, 3, 100, 90), (60, 50, 17, 23),
    (0, 0, W, H), (W - 25, 7, 25, 30), (9, H - 31, 70, 31), (W - 1, H - 1, 1, 1), (W - 64, H - 64, 64, 64),
    (33, 21, 64, 64), (50, 60, 1, 1), (20, 10, 3, 50), (15, 70, 50, 3), (0, 0, 1, 1),
], np.int32)


def _frame(channels, seed, h=H, w=W, pad=13):
    """An (h, w[, c]) view with a row stride larger than w * c inside a random buffer."""
    rng = np.random.default_rng(seed)
    shape = (h, w + pad) if channels == 1 else (h, w + pad, channels)
    buf = rng.integers(0, 256, shape, dtype=np.uint8)
    f = buf[:, :w]
    assert f.strides[0] > w * channels
    return f


def _crops(frame, rects):
    return [frame[y:y + h, x:x + w].copy() for x, y, w, h in rects]


def _oracle(frame, rects, size=(64, 64), rgb=False):
    out = []
    for c in _crops(frame, rects):
        if c.ndim == 3:
            c = c[..., :3][..., ::-1] if rgb else c[..., :3]
        out.append(io.preprocess(c, size))
    return np.stack(out)


@pytest.mark.parametrize("channels,rgb", [(1, False), (3, False), (3, True), (4, False)])
def test_rows_equal_the_crops(eng, channels, rgb):
    frame = _frame(channels, 10 + channels)
    got = eng.preprocess_rois(frame, RECTS, (64, 64), rgb=rgb)
    assert got.shape == (len(RECTS), 4096) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, _oracle(frame, RECTS, rgb=rgb))
    np.testing.assert_array_equal(got, eng.preprocess(_crops(frame, RECTS), (64, 64), rgb=rgb))


def test_non_square_output_and_exact_2x(eng):
    frame = _frame(3, 21)
    got = eng.preprocess_rois(frame, RECTS, (48, 20))
    np.testing.assert_array_equal(got, _oracle(frame, RECTS, (48, 20)))
    np.testing.assert_array_equal(got, eng.preprocess(_crops(frame, RECTS), (48, 20)))
    # 128 x 128 -> 64 x 64 is the INTER_AREA shortcut; its neighbours differ by one pixel from it
    big = _frame(1, 22, 140, 150)
    rects = np.array([(11, 7, 128, 128), (22, 12, 128, 128), (10, 7, 129, 128), (0, 0, 128, 127)], np.int32)
    got = eng.preprocess_rois(big, rects)
    np.testing.assert_array_equal(got, _oracle(big, rects))
    np.testing.assert_array_equal(got, eng.preprocess(_crops(big, rects)))
    from eigenface.image import preprocess_rois
    np.testing.assert_array_equal(preprocess_rois(big, rects), got)


def test_device_frame_and_device_rectangles(eng):
    import torch
    frame = _frame(3, 31)
    buf = torch.as_tensor(np.ascontiguousarray(frame.base), device="cuda")
    dframe = buf[:, :W]  # the same strided view on the device
    assert dframe.stride(0) > W * 3
    rects = np.concatenate([RECTS, np.array([
        (-3, 10, 30, 30),            # negative origin: zero row
        (10, -1, 30, 30),
        (40, 40, 0, 20),             # empty: zero row
        (40, 40, 20, -5),
        (W, 10, 5, 5),               # starts past the frame: zero row
        (W - 20, H - 30, 64, 64),    # overhangs: the clipped crop
        (100, 5, 2 ** 31 - 1, 2 ** 31 - 1),
        (7, 80, 50, 1000),
    ], np.int64).astype(np.int32)])
    got = eng.preprocess_rois(dframe, torch.as_tensor(rects, device="cuda"))
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    n = len(RECTS)
    np.testing.assert_array_equal(got[:n], _oracle(frame, RECTS))
    assert not got[n:n + 5].any()
    clipped = np.array([(W - 20, H - 30, 20, 30), (100, 5, W - 100, H - 5), (7, 80, 50, H - 80)], np.int32)
    np.testing.assert_array_equal(got[n + 5:], _oracle(frame, clipped))
    # host rectangles with a device frame, into a caller's tensor
    out = torch.empty((n, 4096), dtype=torch.uint8, device="cuda")
    assert eng.preprocess_rois(dframe, RECTS, out=out) is out
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), got[:n])


@pytest.mark.parametrize("bad", [(-1, 0, 5, 5), (0, -1, 5, 5), (0, 0, 0, 5), (0, 0, 5, 0), (W - 4, 0, 5, 5),
                                 (0, H - 4, 5, 5), (0, 0, 2 ** 31 - 1, 5)])
def test_bad_host_rectangles_raise(eng, bad):
    from eigenface import EigenfaceError
    frame = _frame(1, 41)
    with pytest.raises(EigenfaceError, match="rectangle 1"):
        eng.preprocess_rois(frame, np.array([(0, 0, 5, 5), bad], np.int32))
    # and the next good call is right
    np.testing.assert_array_equal(eng.preprocess_rois(frame, RECTS[:2]), _oracle(frame, RECTS[:2]))


def test_frames_that_are_not_uint8_raise(eng):
    import torch
    for f in (np.zeros((20, 20), np.float32), np.zeros((20, 20, 3), np.int16),
              torch.zeros((20, 20), dtype=torch.float32, device="cuda")):
        with pytest.raises(TypeError, match="uint8"):
            eng.preprocess_rois(f, np.array([(0, 0, 5, 5)], np.int32))


def test_no_rectangles(eng):
    import torch
    frame = _frame(1, 51)
    assert eng.preprocess_rois(frame, np.zeros((0, 4), np.int32)).shape == (0, 4096)
    d = eng.preprocess_rois(torch.as_tensor(np.ascontiguousarray(frame), device="cuda"),
                            torch.zeros((0, 4), dtype=torch.int32, device="cuda"))
    assert tuple(d.shape) == (0, 4096)
