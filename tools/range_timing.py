#!/usr/bin/env python3
"""Time of the range search next to the score census, on one GPU.

Times, in one process and interleaved inside every repeat, on device tensors and one resident
gallery per case:

  * Engine.search_range_counts(Q, t, metric): the count-only call (one pass of the kernel);
  * Engine.search_range(Q, t, metric, out=...): the filled call (count pass, offset scan, fill
    pass) into the caller's tensors, with no host wait;
  * the yardstick: Engine.score_census of the same probes against the same gallery at 256 bins
    (the identities as labels),

for --probes x --rows x k = 128 and both metrics, at two densities: --per-person rows per identity
(default 8: a handful of hits per probe) and --dense-per-person (default 1000: the cost of the
stores).  The gallery is centres 4 sigma apart per component plus unit noise, a probe is one more
draw around a random row's centre, and the threshold lies between the within- and the
between-identity scores, so a probe's hits are its identity's rows.

Every figure is device time from events on the launch stream, the median of R repeats after
warm-up, with the spread (min, max).  One JSON line per measurement goes to stdout and, with --out,
to a file.
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


def timed(torch, fns, warmup, repeats):
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
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: (float(np.median(v)), float(min(v)), float(max(v))) for name, v in ms.items()}


def case(torch, dev, n, b, k, per_person):
    """(G, identity labels of the rows, Q, identity labels of the probes, {metric: threshold})"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321 + n + per_person)
    lab = (torch.arange(n, device=dev) // per_person).to(torch.int32)
    centres = 4.0 * torch.randn((int(lab.max()) + 1, k), generator=gen, device=dev)
    G = (centres[lab.long()] + torch.randn((n, k), generator=gen, device=dev)).contiguous()
    plab = lab[torch.randint(0, n, (b,), generator=gen, device=dev)]
    Q = (centres[plab.long()] + torch.randn((b, k), generator=gen, device=dev)).contiguous()
    # within an identity |a - b|^2 ~ 2 k and cosine ~ 16 / 17; between ~ 34 k and ~ 0
    return G, lab, Q, plab.contiguous(), {"l2": 4.0 * k, "cosine": 0.55}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--per-person", type=int, default=8)
    ap.add_argument("--dense-per-person", type=int, default=1000, help="0 skips the dense case")
    ap.add_argument("--metrics", default="l2,cosine")
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-census", action="store_true", help="skip the yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("range_timing.py: the median is taken over at least 5 repeats")
    sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))

    import torch
    if not torch.cuda.is_available():
        sys.exit("range_timing.py: no GPU (this tool measures; it has no CPU mode)")
    from eigenface import Engine
    from eigenface.neighbors import search_range_plan

    fh = open(args.out, "a") if args.out else None
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    n, b, k = args.rows, args.probes, args.k
    for per_person in [p for p in (args.per_person, args.dense_per_person) if p > 0]:
        G, lab, Q, plab, thr = case(torch, dev, n, b, k, per_person)
        eng.set_gallery(G)
        eng.set_gallery_labels(lab)
        counts = torch.empty((2, args.bins + 3), dtype=torch.int64, device=dev)
        chunks, tpi = search_range_plan(b, n, k)
        for metric in args.metrics.split(","):
            t = thr[metric]
            total = int(eng.search_range_counts(Q, t, metric)[1][0])  # sizes the outputs, outside the timing
            rows = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            scores = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            infos = {}

            def count(metric=metric, t=t):
                infos["count"] = eng.search_range_counts(Q, t, metric)[1]

            def fill(metric=metric, t=t):
                infos["fill"] = eng.search_range(Q, t, metric, out=(rows, scores)).info

            def census(metric=metric):
                rng = (0.0, 64.0 * k) if metric == "l2" else (-1.0, 1.0)
                eng.score_census(Q, plab, None, metric, args.bins, rng, counts=counts)

            fns = {"count": count, "fill": fill}
            if not args.no_census:
                fns["census"] = census
            res = timed(torch, fns, args.warmup, args.repeats)
            for what, (med, lo, hi) in res.items():
                rec = {"per_person": per_person, "rows": n, "probes": b, "k": k, "metric": metric, "threshold": t,
                       "what": what, "ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                       "repeats": args.repeats, "chunks": chunks, "tiles_per_item": tpi,
                       "pairs_per_s": round(n * b / (med * 1e-3), 1)}
                if what in infos:
                    i = infos[what].cpu().numpy()
                    rec.update(hits=int(i[0]), hits_per_probe=round(int(i[0]) / b, 2), fp64_pairs=int(i[1]),
                               not_written=int(i[2]))
                if "census" in res:
                    rec["census_time_ratio"] = round(med / res["census"][0], 4)
                emit(rec, fh)
        del G, lab, Q, plab
    eng.close()


if __name__ == "__main__":
    main()
