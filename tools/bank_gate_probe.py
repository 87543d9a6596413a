#!/usr/bin/env python3
"""The model bank's face gate against the per-model loop (DESIGN.md "Model bank").

For each shape of tools/bank_probe.py (b faces, M models of k components and n = k gallery rows,
d = 4096 uint8 pixels) three calls:

  bank    one bank_recognize call on the resident bank                       (a)
  gated   one bank_recognize_gated call on the same bank, relative gate 0.1  (b)
  loop    set_model + set_reconstruction + face_distance per model on one Engine: the only way
          to the distances from face space without the grouped form          (c)

All are wall time per call with host arrays in and out, synchronisation included, timed in
alternating batches after a warm-up; the table gives the median batch and the spread.  The
grouped residual GEMM and its reduce are also timed by device events (ef_timing_*), beside the
grouped projection, against one pass over every R at the HBM rate measured for a float4 copy
(MI355X: 6.29 TB/s).

  python tools/bank_gate_probe.py [--out FILE] [--batches 7] [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bank_probe import D, HBM_BYTES_PER_S, per_call  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table and the JSON lines here")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--batch-seconds", type=float, default=0.25)
    ap.add_argument("--quick", action="store_true", help="one small shape (a rehearsal)")
    a = ap.parse_args()

    from eigenface import Engine, bank_recon_schedule
    eng = Engine(0)  # fails without a GPU: there is nothing to measure elsewhere
    rng = np.random.default_rng(0)
    shapes = [(b, m, k) for k in (100, 600) for m in (8, 64) for b in (1, 8, 64)]
    if a.quick:
        shapes = [(8, 4, 100)]
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# gated bank vs ungated bank vs per-model face_distance loop, d = {D} uint8, n = k, wall ms per call "
         f"(median of {a.batches} batches, min .. max), device-event ms, byte floor of every R at "
         f"{HBM_BYTES_PER_S / 1e12:.2f} TB/s")
    emit("#   b    M    k | bank ms (min .. max) | gated ms (min .. max) | gate +ms | loop ms (min .. max) | loop/gated | "
         "nsplit | project ms | residual ms  floor ms  frac  / project | reduce ms")
    for b, m, k in shapes:
        n = k
        mus = [rng.uniform(60, 200, D).astype(np.float32) for _ in range(m)]
        w = (rng.standard_normal((D, k)) / 64).astype(np.float32)  # the same host arrays for every model:
        r = np.ascontiguousarray(w.T)                              # the cost is in bytes, not in values
        s = rng.uniform(0.5, 1.0, D).astype(np.float32)
        g = rng.standard_normal((n, k)).astype(np.float32)
        p = rng.integers(0, 256, (b, D), dtype=np.uint8)
        gate = np.full(m, 0.1, np.float32)

        def loop():
            for mu in mus:
                eng.set_model(mu, w)
                eng.set_reconstruction(r, s)
                eng.face_distance(p, return_energy=True)

        eng.bank_clear()
        for mu in mus:
            eng.bank_set_reconstruction(eng.bank_add(mu, w, g), r, s)

        def bank():
            eng.bank_recognize_raw(p, "cosine")

        def gated():
            eng.bank_recognize_gated_raw(p, gate, "cosine")

        for fn in (loop, bank, gated, loop, bank, gated):  # warm-up: code objects, allocations, tables
            fn()
        tl, tb, tg = [], [], []
        for _ in range(a.batches):  # alternating batches
            tl.append(per_call(loop, a.batch_seconds, 2))
            tb.append(per_call(bank, a.batch_seconds, 5))
            tg.append(per_call(gated, a.batch_seconds, 5))
        # the gated call's kernels by device events, in a pass of their own
        eng.timing(True)
        eng.timing_reset()
        for _ in range(20):
            gated()
        eng.synchronize()
        pj_ms, pj_n = eng.timing_get("project")
        rc_ms, rc_n = eng.timing_get("recon")
        rr_ms, rr_n = eng.timing_get("recon_reduce")
        eng.timing(False)
        eng.timing_reset()
        row = {
            "b": b, "models": m, "k": k, "n": n, "d": D, "nsplit": bank_recon_schedule(b, D, m)["nsplit"],
            "bank_ms": [1e3 * float(np.median(tb)), 1e3 * min(tb), 1e3 * max(tb)],
            "gated_ms": [1e3 * float(np.median(tg)), 1e3 * min(tg), 1e3 * max(tg)],
            "loop_ms": [1e3 * float(np.median(tl)), 1e3 * min(tl), 1e3 * max(tl)],
            "project_ms": pj_ms / max(pj_n, 1), "recon_ms": rc_ms / max(rc_n, 1), "recon_reduce_ms": rr_ms / max(rr_n, 1),
            "recon_floor_ms": 1e3 * m * D * k * 4 / HBM_BYTES_PER_S, "timed_launches": [pj_n, rc_n, rr_n],
        }
        row["gate_ms"] = row["gated_ms"][0] - row["bank_ms"][0]
        row["ratio"] = row["loop_ms"][0] / row["gated_ms"][0]
        emit("{b:5d} {models:4d} {k:4d} | {t[0]:7.3f} ({t[1]:.3f} .. {t[2]:.3f}) | {g[0]:7.3f} ({g[1]:.3f} .. {g[2]:.3f}) | "
             "{gate_ms:7.3f} | {l[0]:8.3f} ({l[1]:.3f} .. {l[2]:.3f}) | {ratio:6.1f} | {nsplit:3d} | {project_ms:8.4f} | "
             "{recon_ms:8.4f} {recon_floor_ms:8.4f} {rf:5.2f} {rp:5.2f} | {recon_reduce_ms:7.4f}".format(
                 t=row["bank_ms"], g=row["gated_ms"], l=row["loop_ms"], rf=row["recon_floor_ms"] / row["recon_ms"],
                 rp=row["recon_ms"] / row["project_ms"], **row))
        lines.append("JSON " + json.dumps(row))
    eng.bank_clear()
    eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
