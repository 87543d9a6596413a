#!/usr/bin/env python3
"""Cost of the Fisher discriminant's two calls (DESIGN.md "Fisher discriminant") on one GPU,
and of the same computation in numpy / scipy fp64 on the host.

One step per process, so that each runs under a time limit of its own:

    timeout -k 10 300 python tools/lda_time.py scatter --out lda_time.jsonl && \
    timeout -k 10 300 python tools/lda_time.py fit --out lda_time.jsonl && \
    timeout -k 10 600 python tools/lda_time.py host --out lda_time.jsonl

scatter / fit: Engine.lda_scatter / Engine.lda_fit on device tensors (float32 features) at
n = 1M, k = 128, C = 10 000 by default; events on the engine's stream around each call, the
median of --runs calls after --warmup, with the spread.  The calls group the labels on the host
and wait for the device, so the figure is the whole call.  The scatter's line also gives the
bytes its passes must move (the features once for the class sums and once per 64-column
operand of each output tile of the scatter product, the order and the labels) and the rate
that makes against the HBM figure.
host: the same statistics and eigenproblem with numpy (sort by label, np.add.reduceat, one
centred GEMM) and scipy.linalg.eigh on the BLAS threads the environment allows.
One JSON line per measurement goes to stdout and, with --out, is appended to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HBM_PEAK = 8.0e12  # bytes/s, the data-sheet figure


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def make_case(n, k, C, seed=0):
    """float32 features with identity centres and a shared 3-direction nuisance, labels
    interleaved; every class has rows."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, C, n).astype(np.int32)
    lab[:C] = np.arange(C)
    u, _ = np.linalg.qr(rng.standard_normal((k, 3)))
    f = (0.5 * rng.standard_normal((C, k), dtype=np.float32))[lab]
    f += 0.4 * rng.standard_normal((n, k), dtype=np.float32)
    f += (8.0 * rng.standard_normal((n, 3), dtype=np.float32)) @ u.T.astype(np.float32)
    return f, lab


def scatter_bytes(n, k, esz):
    nt = (k + 63) // 64
    operand_cols = sum(min(64, k - 64 * a) + min(64, k - 64 * b) for a in range(nt) for b in range(a, nt))
    return n * k * esz + n * operand_cols * esz + n * (8 + 4 + 4)


def gpu_step(what, a):
    sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))
    import torch
    from eigenface import Engine
    f, lab = make_case(a.n, a.k, a.classes)
    with Engine(0) as e:
        stream = torch.cuda.ExternalStream(e.stream_handle(), device=0)
        F = torch.as_tensor(f, device="cuda")
        L = torch.as_tensor(lab, device="cuda")
        torch.cuda.synchronize()
        call = (lambda: e.lda_scatter(F, L, n_classes=a.classes)) if what == "scatter" else \
            (lambda: e.lda_fit(F, L, a.components, n_classes=a.classes))
        ms = []
        for i in range(a.warmup + a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            if i >= a.warmup:
                ms.append(t0.elapsed_time(t1))
    rec = {"step": what, "n": a.n, "k": a.k, "classes": a.classes, "runs": a.runs, "ms_median": float(np.median(ms)),
           "ms_min": min(ms), "ms_max": max(ms)}
    if what == "scatter":
        b = scatter_bytes(a.n, a.k, 4)
        rec.update(bytes=b, passes=b / (a.n * a.k * 4), bytes_per_s=b / (rec["ms_median"] * 1e-3),
                   hbm_fraction=b / (rec["ms_median"] * 1e-3) / HBM_PEAK)
    return rec


def host_step(a):
    import scipy.linalg
    f, lab = make_case(a.n, a.k, a.classes)
    ms = {"scatter": [], "solve": []}
    for i in range(1 + a.host_runs):
        t0 = time.perf_counter()
        x = f.astype(np.float64)
        o = np.argsort(lab, kind="stable")
        cnt = np.bincount(lab, minlength=a.classes)
        starts = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        m = x.mean(axis=0)
        M = np.add.reduceat(x[o], starts, axis=0) / cnt[:, None]
        xc = x - M[lab]
        Sw = xc.T @ xc
        d = M - m
        Sb = d.T @ (d * cnt[:, None])
        t1 = time.perf_counter()
        w, v = scipy.linalg.eigh(Sb, Sw)
        A = v[:, ::-1][:, :a.components] * np.sqrt(a.n - a.classes)
        t2 = time.perf_counter()
        if i:
            ms["scatter"].append((t1 - t0) * 1e3)
            ms["solve"].append((t2 - t1) * 1e3)
    return {"step": "host", "n": a.n, "k": a.k, "classes": a.classes, "runs": a.host_runs,
            "threads": os.environ.get("OMP_NUM_THREADS", ""), "scatter_ms_median": float(np.median(ms["scatter"])),
            "solve_ms_median": float(np.median(ms["solve"])), "checksum": float(np.abs(A).sum())}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("step", choices=["scatter", "fit", "host"])
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--k", type=int, default=128)
    p.add_argument("--classes", type=int, default=10_000)
    p.add_argument("--components", type=int, default=64)
    p.add_argument("--runs", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--host-runs", type=int, default=3)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    emit(host_step(a) if a.step == "host" else gpu_step(a.step, a), a.out)


if __name__ == "__main__":
    main()
