"""Context lifecycle (DESIGN.md "Ownership"): a failed ef_tm_prepare leaves no half-built
localiser behind, create / use / trim / destroy cycles give their device memory back, and
every buffer ef_trim frees is rebuilt on the next call with the same results."""
import ctypes as C

import numpy as np
import pytest

import jpeg_cases as J
from eigenface import _native as N
from oracle import eigenface_oracle as orc

pytestmark = pytest.mark.gpu

MIB = 1 << 20
EF_E_INVALID, EF_E_STATE = -1, -3  # include/eigenface.h


def _tm_problem():
    rng = np.random.default_rng(5)
    frame = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    templ = frame[20:32, 30:40].copy()  # 12 x 10 (h x w), cut from the frame at x = 30, y = 20
    return frame, templ


def _jpeg_pair():
    return [J.encode(J.smooth_image(64, 64, 3, 11), quality=85, subsampling=2),
            J.encode(J.smooth_image(33, 47, 1, 12), quality=80)]


def test_failed_prepare_leaves_no_state(eng):
    frame, templ = _tm_problem()
    eng.tm_prepare([templ], [(0, 12, 10)], frame.shape)
    best0, x0, y0 = eng.tm_match(frame)
    assert (int(x0[0]), int(y0[0])) == (30, 20)
    with pytest.raises(N.EigenfaceError) as ei:
        eng.tm_prepare([templ, np.zeros((0, 10), np.uint8)], [(0, 12, 10)], frame.shape)
    assert ei.value.code == EF_E_INVALID
    # the context has no localiser now (nothing is launched on the failed state)
    n, tot = C.c_int32(0), C.c_int64(0)
    assert eng._lib.ef_tm_info(eng._h, C.byref(n), C.byref(tot), None, None) == EF_E_STATE
    eng.tm_prepare([templ], [(0, 12, 10)], frame.shape)
    best1, x1, y1 = eng.tm_match(frame)
    np.testing.assert_array_equal(best1, best0)
    np.testing.assert_array_equal(x1, x0)
    np.testing.assert_array_equal(y1, y0)


def test_context_cycles_return_memory(eng):
    """Ten create / use / trim / destroy cycles beside the session context.  The smallest
    buffer that exists only through these calls is the 4 MiB prefix copy of the gallery
    (65536 x 16 floats): leaked once per cycle it costs 32 MiB between cycles 2 and 10, so
    free device memory may drop by less than 16 MiB."""
    import torch
    from eigenface import Engine
    rng = np.random.default_rng(9)
    g = rng.standard_normal((65536, 32)).astype(np.float32)
    q = (g[rng.integers(0, len(g), 256)] + 0.05 * rng.standard_normal((256, 32))).astype(np.float32)
    x, _ = orc.synth_faces(900, 16, r=32, seed=21)  # 900 x 256
    frame, templ = _tm_problem()
    blobs = _jpeg_pair()

    def cycle():
        with Engine(0) as e:
            e.set_gallery(g)
            e.set_option("search_prefix", 16)
            k_prefix = e.search_keys(q, "l2")
            assert e.search_stats()[1] + e.search_stats()[2] == 256  # the prefix scan ran
            e.set_option("search_split_bf16", 1)
            k_split = e.search_keys(q, "l2")
            fit = e.fit(x, 10)
            e.tm_prepare([templ], [(0, 12, 10)], frame.shape)
            _, tx, ty = e.tm_match(frame)
            imgs = e.decode_jpegs(blobs, "bgr")
            e.trim()
        return k_prefix, k_split, fit.components, (int(tx[0]), int(ty[0])), imgs

    free = {}
    first = last = None
    for i in range(1, 11):
        last = cycle()
        if i == 1:
            first = last
        if i in (2, 10):
            torch.cuda.synchronize()
            free[i] = torch.cuda.mem_get_info(0)[0]
    drop = free[2] - free[10]
    print(f"free device memory after cycle 2: {free[2] / MIB:.1f} MiB, after cycle 10: {free[10] / MIB:.1f} MiB, "
          f"drop {drop / MIB:.2f} MiB")
    np.testing.assert_array_equal(last[0], first[0])
    np.testing.assert_array_equal(last[1], first[1])
    np.testing.assert_array_equal(last[2], first[2])
    assert last[3] == first[3] == (30, 20)
    for a, b in zip(last[4], first[4]):
        np.testing.assert_array_equal(a, b)
    assert drop < 16 * MIB


def test_trim_then_reuse():
    """ef_trim frees the fit pool, the JPEG workspaces and the pinned upload slots; the next
    decode and fit on the same context rebuild them and give byte-identical results."""
    from eigenface import Engine
    x, _ = orc.synth_faces(900, 16, r=32, seed=21)
    blobs = _jpeg_pair()
    with Engine(0) as e:
        imgs0 = e.decode_jpegs(blobs, "bgr")
        rows0, st0 = e.ingest_jpegs(blobs, (32, 32), "gray")
        fit0 = e.fit(x, 10)
        e.trim()
        imgs1 = e.decode_jpegs(blobs, "bgr")
        rows1, st1 = e.ingest_jpegs(blobs, (32, 32), "gray")
        fit1 = e.fit(x, 10)
        e.trim()
        e.trim()  # nothing left to free
    assert imgs0[0].shape == (64, 64, 3) and imgs0[1].shape == (33, 47, 3)
    for a0, a1 in zip(imgs0, imgs1):
        np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(st1, st0)
    np.testing.assert_array_equal(rows1, rows0)
    np.testing.assert_array_equal(fit1.components, fit0.components)
    np.testing.assert_array_equal(fit1.projection, fit0.projection)
    np.testing.assert_array_equal(fit1.mean, fit0.mean)
