#!/usr/bin/env python3
"""Time of the gallery clustering next to the score census, on one GPU.

Times, in one process and interleaved inside every repeat, on device tensors and one resident
gallery per case:

  * Engine.cluster_gallery(threshold, metric): the link pass alone (min_samples = 1);
  * Engine.cluster_gallery(threshold, metric, min_samples = 4): the count pass over the full
    square, then the link pass;
  * the yardstick: a self-join of the same gallery through Engine.score_census, every row a probe
    with its own row excluded, in 4096-probe batches (1024 bins, the identities as labels),

for 262 144 and 1 000 000 rows x k = 128 and both metrics, at two densities: all singletons (random
rows, nothing within the threshold) and about 1000 rows per identity (centres 4 sigma apart per
component plus unit noise, the threshold between the within- and between-identity scores).  A third
density, every row identical at 65 536 rows, is the union-find's worst case: every pair is an edge.

Pair-visits: the census visits n^2 ordered pairs, the link pass n_t (n_t + 1) / 2 tiles of 128 x 128
(half of them), the count pass n_t^2 tiles.  Every figure is device time from events on the launch
stream, the median of R repeats after warm-up, with the spread (min, max).  One JSON line per
measurement goes to stdout and, with --out, to a file.
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


def gallery(torch, dev, density, n, k, per_person):
    """(G, identity labels, {metric: threshold})"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234 + n)
    if density == "singletons":
        G = torch.randn((n, k), generator=gen, device=dev)
        lab = torch.arange(n, dtype=torch.int32, device=dev)
        return G, lab, {"l2": 1.0, "cosine": 0.9}  # |a - b|^2 ~ 2 k, cosine ~ N(0, 1/k)
    if density == "identical":
        G = torch.randn((1, k), generator=gen, device=dev).repeat(n, 1).contiguous()
        return G, torch.zeros(n, dtype=torch.int32, device=dev), {"l2": 0.5, "cosine": 0.5}
    lab = (torch.arange(n, device=dev) // per_person).to(torch.int32)
    centres = 4.0 * torch.randn((int(lab.max()) + 1, k), generator=gen, device=dev)
    G = centres[lab.long()] + torch.randn((n, k), generator=gen, device=dev)
    # within an identity |a - b|^2 ~ 2 k and cosine ~ 16 / 17; between ~ 34 k and ~ 0
    return G.contiguous(), lab, {"l2": 4.0 * k, "cosine": 0.55}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="262144,1000000", help="comma-separated row counts of the two open densities")
    ap.add_argument("--identical-rows", type=int, default=65536)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--per-person", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=4096, help="probes per score_census call of the yardstick")
    ap.add_argument("--metrics", default="l2,cosine")
    ap.add_argument("--densities", default="singletons,identities,identical")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-census", action="store_true", help="skip the yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("cluster_timing.py: the median is taken over at least 5 repeats")
    sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))

    import torch
    if not torch.cuda.is_available():
        sys.exit("cluster_timing.py: no GPU (this tool measures; it has no CPU mode)")
    from eigenface import Engine

    fh = open(args.out, "a") if args.out else None
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    k = args.k
    cases = [(d, int(n)) for d in args.densities.split(",") if d != "identical" for n in args.rows.split(",")]
    if "identical" in args.densities.split(","):
        cases.append(("identical", args.identical_rows))
    for density, n in cases:
        G, lab, thr = gallery(torch, dev, density, n, k, args.per_person)
        eng.set_gallery(G)
        eng.set_gallery_labels(lab)
        rows = torch.arange(n, dtype=torch.int64, device=dev)
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        degree = torch.empty(n, dtype=torch.int32, device=dev)
        counts = torch.empty((2, 1024 + 3), dtype=torch.int64, device=dev)
        tiles = (n + 127) // 128
        visits = {"link": tiles * (tiles + 1) // 2 * 128 * 128, "count+link": (tiles * tiles + tiles * (tiles + 1) // 2) * 128 * 128,
                  "census": n * n}
        for metric in args.metrics.split(","):
            t = thr[metric]
            infos = {}

            def link(metric=metric, t=t):
                infos["link"] = eng.cluster_gallery(t, metric, 1, labels=labels)[2]

            def both(metric=metric, t=t):
                infos["count+link"] = eng.cluster_gallery(t, metric, 4, degree=degree, labels=labels)[2]

            def census(metric=metric):
                rng = (0.0, 64.0 * k) if metric == "l2" else (-1.0, 1.0)
                for a in range(0, n, args.batch):
                    s = slice(a, min(n, a + args.batch))
                    eng.score_census(G[s], lab[s], rows[s], metric, 1024, rng, counts=counts)

            fns = {"link": link, "count+link": both}
            if not args.no_census:
                fns["census"] = census
            res = timed(torch, fns, args.warmup, args.repeats)
            for what, (med, lo, hi) in res.items():
                rec = {"density": density, "rows": n, "k": k, "metric": metric, "threshold": t, "what": what,
                       "ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3), "repeats": args.repeats,
                       "pair_visits": visits[what], "pair_visits_per_s": round(visits[what] / (med * 1e-3), 1)}
                if what in infos:
                    i = infos[what].cpu().numpy()
                    rec.update(clusters=int(i[0]), noise=int(i[1]), links=int(i[2]), fp64_pairs=int(i[3] & ((1 << 62) - 1)),
                               unconverged=bool(i[3] >> 62))
                if "census" in res:
                    rec["census_time_ratio"] = round(med / res["census"][0], 4)
                    rec["census_rate_ratio"] = round((visits[what] / med) / (visits["census"] / res["census"][0]), 4)
                emit(rec, fh)
        del G, lab
    eng.close()


if __name__ == "__main__":
    main()
