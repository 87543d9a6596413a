#!/usr/bin/env python3
"""Time of the score census next to the labelled scan, on one GPU.

Times, in one process and interleaved inside every repeat, on device tensors and the same
resident labelled gallery:

  * Engine.search_labelled_keys(..., "other") with an excluded row per probe: one labelled
    fp32 scan, the yardstick;
  * Engine.score_census with the same probes, labels and excluded rows, per bin count,

at 4096 probes against 1M x 128 rows by default, for L2 and cosine.  The gallery is stored
person by person (label = row // per-person); every probe is a noisy copy of a gallery row and
carries that row's label and index.  The census range is evaluate.score_census's default: (-1, 1)
for cosine, (0, 4 max ||g||^2) for L2.

Every figure is device time from events on the launch stream around K back-to-back calls, the
median of R repeats after warm-up, with the spread (min, max).  One JSON line per measurement
goes to stdout and, with --out, to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


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
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--per-person", type=int, default=1000)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--metrics", default="l2,cosine")
    ap.add_argument("--nbins", default="1024", help="comma-separated bin counts")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("census_timing.py: the median is taken over at least 5 repeats")
    sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))

    import torch
    if not torch.cuda.is_available():
        sys.exit("census_timing.py: no GPU (this tool measures; it has no CPU mode)")
    from eigenface import Engine, synth
    from eigenface.evaluate import _default_census_range

    fh = open(args.out, "a") if args.out else None
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    k = args.k
    G = synth.gallery_rows(0, args.rows, k)
    targets = np.random.default_rng(2024).integers(0, args.rows, args.probes)
    rng = np.random.default_rng(5)
    Q = G[targets] + 0.05 * rng.standard_normal((args.probes, k)).astype(np.float32) * synth.spectrum(k).astype(np.float32)
    glab = (np.arange(args.rows) // args.per_person).astype(np.int32)
    Gd, Qd = torch.from_numpy(G).to(dev), torch.from_numpy(Q).to(dev)
    eng.set_gallery(Gd)
    eng.set_gallery_labels(torch.from_numpy(glab).to(dev))
    pl = torch.from_numpy(glab[targets]).to(dev)
    ex = torch.from_numpy(targets.astype(np.int64)).to(dev)
    keys = torch.empty(args.probes, dtype=torch.int64, device=dev)
    bins = [int(v) for v in args.nbins.split(",") if v]
    base = {"rows": args.rows, "k": k, "probes": args.probes, "steps": args.steps, "repeats": args.repeats}
    for metric in args.metrics.split(","):
        lo_hi = _default_census_range(G, metric)
        fns = {"labelled_other": lambda: eng.search_labelled_keys(Qd, pl, "other", ex, metric, keys=keys)}
        outs = {}
        for nb in bins:
            outs[nb] = torch.empty((2, nb + 3), dtype=torch.int64, device=dev)
            fns[f"census_{nb}"] = (lambda nb=nb: eng.score_census(Qd, pl, ex, metric, nb, lo_hi, counts=outs[nb]))
        res = timed(torch, fns, args.steps, args.warmup, args.repeats)
        scan = res["labelled_other"][0]
        for what, (med, lo, hi) in res.items():
            rec = {**base, "metric": metric, "what": what, "ms": round(med, 4), "min_ms": round(lo, 4),
                   "max_ms": round(hi, 4), "labelled_scans": round(med / scan, 4)}
            if what.startswith("census_"):
                c = outs[int(what.split("_")[1])].cpu().numpy()
                rec.update(range=list(lo_hi), pairs=int(c.sum()), occupied_slots=int((c > 0).sum()),
                           tflops=round(2.0 * k * args.probes * args.rows / (med * 1e-3) / 1e12, 2))
            emit(rec, fh)
    eng.close()


if __name__ == "__main__":
    main()
