#!/usr/bin/env python3
"""Device time of ef_face_distance next to ef_project.

Device-resident uint8 probes; per shape the two calls alternate, each bracketed by a pair of
HIP events on the stream the engine launches on, after a warm-up; the medians are reported.
A second pass with the library's device timers on gives the kernels' own times: project_kernel
(EF_KERNEL_PROJECT), the residual GEMM (EF_KERNEL_RECON) and its reduce (EF_KERNEL_RECON_REDUCE).
ef_face_distance contains ef_project's whole sequence, so `added` = distance - project is what
the back-projection costs.  Prints one JSON line per shape; needs a GPU.

    python tools/recon_bench.py [--reps 40] [--warmup 5] [--shapes c3,scanner] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))

SHAPES = {"c3": (4096, 16384, 128), "scanner": (64, 4096, 50)}


def bench(eng, torch, name, b, d, k, reps, warmup):
    rng = np.random.default_rng(0)
    q, _ = np.linalg.qr(rng.standard_normal((d, k)))
    V = np.ascontiguousarray(q.T, dtype=np.float32)
    mean = rng.uniform(100, 156, d).astype(np.float32)
    eng.set_model(mean, np.ascontiguousarray(V.T))
    eng.set_reconstruction(V)
    dev = torch.device("cuda", eng.device)
    P = torch.from_numpy(rng.integers(0, 256, (b, d), dtype=np.uint8)).to(dev)
    F = torch.empty((b, k), dtype=torch.float32, device=dev)
    E = torch.empty((b,), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(eng.device)
    eng.set_stream(stream.cuda_stream)  # the events below bracket exactly the engine's work
    calls = {"project": lambda: eng.project(P, out=F), "distance": lambda: eng.face_distance(P, out=E)}
    times = {n: [] for n in calls}
    try:
        for it in range(warmup + reps):
            for n, fn in calls.items():
                a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                fn()
                z.record(stream)
                z.synchronize()
                if it >= warmup:
                    times[n].append(a.elapsed_time(z))
        eng.timing_reset()
        eng.timing(True)
        for _ in range(reps):
            eng.face_distance(P, out=E)
        eng.synchronize()
        kern = {n: eng.timing_get(n) for n in ("project", "recon", "recon_reduce")}
    finally:
        eng.timing(False)
        eng.timing_reset()
        eng.use_own_stream()
    med = {n: float(np.median(v)) for n, v in times.items()}
    res = {"shape": name, "b": b, "d": d, "k": k, "reps": reps,
           "project_call_ms": med["project"], "distance_call_ms": med["distance"],
           "added_ms": med["distance"] - med["project"], "distance_over_project": med["distance"] / med["project"],
           "call_spread_ms": {n: [float(np.min(v)), float(np.max(v))] for n, v in times.items()}}
    for n, (ms, cnt) in kern.items():
        res[f"{n}_kernel_ms"] = ms / max(cnt, 1)
    res["recon_over_project_kernel"] = res["recon_kernel_ms"] / res["project_kernel_ms"]
    # what the residual pass has to move and compute
    flop = 2.0 * b * d * k
    res["recon_tflops"] = flop / (res["recon_kernel_ms"] * 1e-3) / 1e12
    res["project_tflops"] = flop / (res["project_kernel_ms"] * 1e-3) / 1e12
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="c3,scanner", help="comma-separated: " + ", ".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("recon_bench: no GPU (this measurement has no CPU form)")
    from eigenface import Engine
    lines = []
    with Engine(0) as eng:
        for name in args.shapes.split(","):
            b, d, k = SHAPES[name]
            lines.append(json.dumps(bench(eng, torch, name, b, d, k, args.reps, args.warmup)))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
