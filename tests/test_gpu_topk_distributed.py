"""ShardedGallery.search_topk_keys across ranks: 2 ranks share the one GPU (gloo for the
all-gather, as in test_gpu_distributed.py), each holds half the gallery, and the merged top-m
keys of every rank must equal one engine's over the whole gallery — through the device merge
(device probes) and through the host merge (host probes)."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import PKG, ROOT
from test_gpu_distributed import _port

pytestmark = pytest.mark.gpu

M = 6


def _rank(rank, world, port, g, q, out):
    import sys
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from eigenface import Engine
    from eigenface.distributed import ShardedGallery, shard_range
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    lo, hi = shard_range(len(g), rank, world)
    sg = ShardedGallery(eng, g[lo:hi], len(g), rank, world)
    res = {}
    for metric in ("l2", "cosine"):
        dev = sg.search_topk_keys(torch.from_numpy(q).cuda(), M, metric)
        assert dev.is_cuda
        res[metric, "device"] = dev.cpu().numpy()
        res[metric, "host"] = np.asarray(sg.search_topk_keys(q, M, metric))
    torch.cuda.synchronize()
    out[rank] = res
    eng.close()
    dist.destroy_process_group()


def test_two_ranks_topk_equals_single_engine(eng):
    rng = np.random.default_rng(21)
    n, k = 4001, 40
    g = rng.standard_normal((n, k)).astype(np.float32)
    g[n - 1] = g[7]  # a duplicate across the shard boundary: 7 before n - 1
    q = rng.standard_normal((130, k)).astype(np.float32)
    q[0] = g[7]
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = _port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, g, q, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    eng.set_option("search_split_bf16", 0)
    eng.set_gallery(g)
    for metric in ("l2", "cosine"):
        ref = eng.search_topk_keys(q, M, metric)
        assert (ref[0, :2] & 0xFFFFFFFF).tolist() == [7, n - 1]
        for r in range(2):
            np.testing.assert_array_equal(out[r][metric, "device"], ref)
            np.testing.assert_array_equal(out[r][metric, "host"], ref)


def test_one_rank_is_the_engine(eng):
    from eigenface.distributed import ShardedGallery
    rng = np.random.default_rng(22)
    g = rng.standard_normal((700, 24)).astype(np.float32)
    q = rng.standard_normal((50, 24)).astype(np.float32)
    sg = ShardedGallery(eng, g, len(g), 0, 1)
    np.testing.assert_array_equal(sg.search_topk_keys(q, 4, "cosine"), eng.search_topk_keys(q, 4, "cosine"))
