#!/usr/bin/env python3
"""Cost of the labelled search next to the plain fp32 scan, on one GPU.

Times, in one process and interleaved inside every repeat, on device tensors:

  * Engine.search_keys with the prefix scan and the split scan off (one plain fp32 top-1
    scan: the unit the ratios are in; with --top1-only this is all the tool runs, and --pkg
    points it at another checkout's package, so the parent commit is timed by the same code);
  * Engine.search_labelled_keys for SAME, OTHER and ANY, each with an excluded row per probe,

at the C3 shape (1M x 128, 4096 probes) and at k = 512, for L2 and cosine.  The gallery is
stored person by person: 1000 people x 1000 rows, label = row // 1000; every probe is a
noisy copy of a gallery row and carries that row's label and index (a leave-one-out probe).
With --loo-rows N it also times a full evaluate.leave_one_out of an N-row gallery (host
arrays in and out, wall clock, batches of 4096).

Every scan figure is device time from events on the launch stream around K back-to-back
calls, the median of R repeats after warm-up, with the spread (min, max).  One JSON line per
measurement goes to stdout and, with --out, to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = {"c3": 128, "c5": 512}


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def timed(torch, fns, steps, warmup, repeats):
    """{name: (median, min, max) ms per call}: the variants run interleaved inside every repeat."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / steps)
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--per-person", type=int, default=1000)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--metrics", default="l2,cosine")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--top1-only", action="store_true", help="time search_keys only (works on older checkouts)")
    ap.add_argument("--once", action="store_true", help="one labelled call per relation, untimed (for a profiler run)")
    ap.add_argument("--loo-rows", type=int, default=0, help="also time leave_one_out of a gallery of this many rows (k = 128)")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "face-detection-recognization-pca_amd"),
                    help="directory holding the eigenface package to measure")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))

    import torch
    if not torch.cuda.is_available():
        sys.exit("labelled_probe.py: no GPU (this tool measures; it has no CPU mode)")
    from eigenface import Engine, synth

    fh = open(args.out, "a") if args.out else None
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_option("search_prefix", 0)
    eng.set_option("search_split_bf16", 0)
    for shape in [s for s in args.shapes.split(",") if s]:
        k = SHAPES[shape]
        t0 = time.perf_counter()
        G = synth.gallery_rows(0, args.rows, k)
        targets = np.random.default_rng(2024).integers(0, args.rows, args.probes)
        rng = np.random.default_rng(5)
        Q = (G[targets] + 0.05 * rng.standard_normal((args.probes, k)).astype(np.float32) * synth.spectrum(k).astype(np.float32))
        glab = (np.arange(args.rows) // args.per_person).astype(np.int32)
        Gd, Qd = torch.from_numpy(G).to(dev), torch.from_numpy(Q).to(dev)
        eng.set_gallery(Gd)
        keys = torch.empty(args.probes, dtype=torch.int64, device=dev)
        base = {"label": args.label, "shape": shape, "rows": args.rows, "k": k, "probes": args.probes,
                "steps": args.steps, "repeats": args.repeats}
        if not args.top1_only:
            eng.set_gallery_labels(torch.from_numpy(glab).to(dev))
            pl = torch.from_numpy(glab[targets]).to(dev)
            ex = torch.from_numpy(targets.astype(np.int64)).to(dev)
        emit({**base, "what": "setup_s", "value": round(time.perf_counter() - t0, 1)}, fh)
        for metric in args.metrics.split(","):
            if args.once:
                for rel in ("same", "other", "any"):
                    eng.search_labelled_keys(Qd, pl, rel, ex, metric, keys=keys)
                torch.cuda.synchronize()
                continue
            fns = {"top1": lambda: eng.search_keys(Qd, metric, keys=keys)}
            if not args.top1_only:
                for rel in ("same", "other", "any"):
                    fns[f"labelled_{rel}"] = (lambda rel=rel: eng.search_labelled_keys(Qd, pl, rel, ex, metric, keys=keys))
            res = timed(torch, fns, args.steps, args.warmup, args.repeats)
            t1 = res["top1"][0]
            for what, (med, lo, hi) in res.items():
                emit({**base, "metric": metric, "what": what, "ms": round(med, 4), "min_ms": round(lo, 4),
                      "max_ms": round(hi, 4), "top1_scans": round(med / t1, 4)}, fh)
        del Gd, Qd
        torch.cuda.empty_cache()
    if args.loo_rows and not args.top1_only:
        from eigenface import leave_one_out, open_set_rates
        n, k = args.loo_rows, 128
        G = synth.gallery_rows(0, n, k)
        lab = (np.arange(n) // 64).astype(np.int32)
        for metric in args.metrics.split(","):
            wall = []
            for _ in range(3):
                t0 = time.perf_counter()
                loo = leave_one_out(G, lab, metric, engine=eng)
                wall.append(time.perf_counter() - t0)
            emit({"label": args.label, "what": "leave_one_out", "rows": n, "k": k, "metric": metric,
                  "wall_s": round(float(np.median(wall)), 4), "min_s": round(min(wall), 4), "max_s": round(max(wall), 4),
                  "rank1": open_set_rates(loo["genuine_key"], loo["impostor_key"], metric).rank1}, fh)
    eng.close()


if __name__ == "__main__":
    main()
