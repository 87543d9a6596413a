"""The exact integer pieces of include/eigenface.h ef_fit_shard_stats, restated in numpy: the
one definition the CPU tests (test_distributed_cpu.py) and the GPU tests
(test_gpu_shard_stats_exact.py) both hold the library against."""
import numpy as np


def shard_pieces(x):
    """(sum x [d], sum x^2 [d], X'^T X' [d, d] with X' = X - 128) of uint8 rows x (n x d), int64.

    The cross products go through the float64 BLAS product: every entry of X' is an integer
    of magnitude <= 128, so every product and every partial sum of a dot product is an
    integer of magnitude <= n * 2^14 < 2^53 (n < 2^39), exactly representable in float64,
    and the result is the exact integer whatever order BLAS adds in."""
    x = np.asarray(x)
    assert x.ndim == 2 and x.shape[0] < 2 ** 39
    xi = x.astype(np.int64)
    xs = x.astype(np.float64) - 128.0
    return xi.sum(0), (xi * xi).sum(0), (xs.T @ xs).astype(np.int64)


def upper_block_mask(d, block=64):
    """True where (i, j) lies in an upper 64-block (i // 64 <= j // 64): the part of the cross
    products ef_fit_shard_stats defines; the rest is unspecified."""
    b = np.arange(d) // block
    return b[:, None] <= b[None, :]
