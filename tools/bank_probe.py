#!/usr/bin/env python3
"""Model bank against the per-model loop (DESIGN.md "Model bank").

For each shape (b faces, M models of k components and n = k gallery rows, d = 4096 uint8
pixels) two ways of answering "which model knows this face":

  loop   set_model + set_gallery + recognize per model on one Engine, host arrays: what
         compat.recognize_faces_all_models costs per frame apart from its array hashing
  bank   one bank_recognize call on the resident bank, host arrays in and out

Both are wall time per call, synchronisation included (the loop's cost is uploads and
launches).  The two are timed in alternating batches after a warm-up of every shape; the
table gives the median batch and the spread (min .. max) of the per-call time.  The bank's two
kernels are also timed by device events (ef_timing_*) against their byte floor: one pass over
every W and every gallery at the HBM rate measured for a float4 copy (MI355X: 6.29 TB/s).

  python tools/bank_probe.py [--out FILE] [--batches 7] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy; the spec figure is 8.0e12
D = 4096


def per_call(fn, min_s, min_calls):
    """Seconds per call of one batch: calls until min_s have passed, at least min_calls."""
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if n >= min_calls and dt >= min_s:
            return dt / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines here")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.25)
    ap.add_argument("--quick", action="store_true", help="one small shape (a rehearsal)")
    a = ap.parse_args()

    from eigenface import Engine
    eng = Engine(0)  # fails without a GPU: there is nothing to measure elsewhere
    rng = np.random.default_rng(0)
    shapes = [(b, m, k) for k in (100, 600) for m in (8, 64) for b in (1, 8, 64)]
    if a.quick:
        shapes = [(8, 4, 100)]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# model bank vs per-model loop, d = {D} uint8, n = k, wall ms per call (median of {a.batches} batches, "
         f"min .. max), device-event ms of the bank's kernels, byte floor at {HBM_BYTES_PER_S / 1e12:.2f} TB/s")
    emit("#   b    M    k | loop ms (min .. max) | bank ms (min .. max) | ratio | project ms  floor ms  frac | "
         "search ms  floor ms  frac")
    for b, m, k in shapes:
        n = k
        mus = [rng.uniform(60, 200, D).astype(np.float32) for _ in range(m)]
        w = (rng.standard_normal((D, k)) / 64).astype(np.float32)  # the same host array for every model:
        g = rng.standard_normal((n, k)).astype(np.float32)         # the cost is in bytes, not in values
        p = rng.integers(0, 256, (b, D), dtype=np.uint8)

        def loop():
            for mu in mus:
                eng.set_model(mu, w)
                eng.set_gallery(g)
                eng.recognize_keys(p, "cosine")

        eng.bank_clear()
        for mu in mus:
            eng.bank_add(mu, w, g)

        def bank():
            eng.bank_recognize_raw(p, "cosine")

        for fn in (loop, bank, loop, bank):  # warm-up: code objects, allocations, tables
            fn()
        tl, tb = [], []
        for _ in range(a.batches):  # alternating batches
            tl.append(per_call(loop, a.batch_seconds, 2))
            tb.append(per_call(bank, a.batch_seconds, 5))
        # the bank's kernels by device events, in a pass of their own
        eng.timing(True)
        eng.timing_reset()
        calls = 20
        for _ in range(calls):
            bank()
        eng.synchronize()
        pj_ms, pj_n = eng.timing_get("project")
        se_ms, se_n = eng.timing_get("search")
        eng.timing(False)
        eng.timing_reset()
        w_bytes, g_bytes = m * D * k * 4, m * n * k * 4
        row = {
            "b": b, "models": m, "k": k, "n": n, "d": D,
            "loop_ms": [1e3 * float(np.median(tl)), 1e3 * min(tl), 1e3 * max(tl)],
            "bank_ms": [1e3 * float(np.median(tb)), 1e3 * min(tb), 1e3 * max(tb)],
            "project_ms": pj_ms / max(pj_n, 1), "search_ms": se_ms / max(se_n, 1),
            "project_floor_ms": 1e3 * w_bytes / HBM_BYTES_PER_S, "search_floor_ms": 1e3 * g_bytes / HBM_BYTES_PER_S,
            "timed_launches": [pj_n, se_n],
        }
        row["ratio"] = row["loop_ms"][0] / row["bank_ms"][0]
        emit("{b:5d} {models:4d} {k:4d} | {l[0]:8.3f} ({l[1]:.3f} .. {l[2]:.3f}) | {t[0]:7.3f} ({t[1]:.3f} .. {t[2]:.3f}) | "
             "{ratio:5.1f} | {project_ms:8.4f} {project_floor_ms:8.4f} {pf:5.2f} | {search_ms:8.4f} {search_floor_ms:8.4f} "
             "{sf:5.3f}".format(l=row["loop_ms"], t=row["bank_ms"], pf=row["project_floor_ms"] / row["project_ms"],
                                sf=row["search_floor_ms"] / row["search_ms"], **row))
        lines.append("JSON " + json.dumps(row))
    eng.bank_clear()
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
