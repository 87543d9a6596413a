"""ef_fit_shard_stats / Engine.fit_shard_stats against exact integers: the sums of x and x^2
and X'^T X' (X' = X - 128) on every entry of the upper 64-blocks, the documented contract
(include/eigenface.h), host and device forms.  tests/test_gpu_sharded_fit.py holds the same
call against Engine.fit on the same kernels; here the reference is numpy's
(tests/shard_util.py, shared with test_distributed_cpu.py).  The shapes: one pixel and one
row; an empty shard; an order just past one 64-block with ragged K (byte-granular transpose,
d % 4 != 0); the LDS transpose (d % 256 == 0); the 256 x 384 tiles of orders >= 2048."""
import numpy as np
import pytest

from shard_util import shard_pieces, upper_block_mask

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (0, 70), (130, 65), (200, 256), (64, 2050)]


def _pixels(n, d):
    rng = np.random.default_rng(1000 * n + d)
    x = rng.integers(0, 256, (n, d), dtype=np.uint8)
    if n and d >= 3:
        x[:, 1] = 0      # x' = -128: the largest products
        x[:, 2] = 255    # x' = 127
    return x


def _check(pieces, x):
    s1, s2, cr = (p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p) for p in pieces)
    n, d = x.shape
    r1, r2, rc = shard_pieces(x)
    assert s1.dtype == np.int64 and s2.dtype == np.int64 and cr.dtype == np.int64 and cr.shape == (d, d)
    np.testing.assert_array_equal(s1, r1)
    np.testing.assert_array_equal(s2, r2)
    if n == 0:  # an empty shard contributes nothing, anywhere
        assert not s1.any() and not s2.any() and not cr.any()
        return
    m = upper_block_mask(d)
    np.testing.assert_array_equal(cr[m], rc[m])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_shard_stats_are_the_exact_integers(eng, n, d, device):
    x = _pixels(n, d)
    if device:
        import torch
        _check(eng.fit_shard_stats(torch.from_numpy(x).cuda()), x)
    else:
        _check(eng.fit_shard_stats(x), x)


def test_shard_stats_exact_with_one_slab(eng):
    """The slab budget lowered to one slab (one K-split, every stage in one work item)."""
    n, d = 200, 256
    x = _pixels(n, d)
    default = eng.get_option("cov_slab_bytes")
    eng.set_option("cov_slab_bytes", d * d * 4)
    try:
        pieces = eng.fit_shard_stats(x)
    finally:
        eng.set_option("cov_slab_bytes", default)
    _check(pieces, x)
