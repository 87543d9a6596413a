#!/usr/bin/env python3
"""Time of the identification-rank search next to its two yardsticks, on one GPU.

Times, in one process and interleaved inside every repeat, on device tensors and one resident
labelled gallery per regime:

  * rank:        Engine.search_rank(Q, labels, metric=..., out=...): the labelled SAME scan, the
                 thresholds, the rank scan into the bitmap, the popcount;
  * rank_given:  the same call with the genuine records handed in (no labelled scan);
  * the yardsticks, code the rank search does not touch:
      labelled:  Engine.search_labelled_keys(Q, labels, "same", ...);
      count:     Engine.search_range_counts(Q, t, metric) at a threshold between the within- and
                 the between-identity scores,

for --probes x --rows x k = 128, --per-person rows per identity (8: C = 125 000 identities, a 64 MB
bitmap) and both metrics, in two regimes:

  * easy: centres 4 sigma apart per component plus unit noise, a probe one more draw around a
    random identity's centre: the genuine row comes first, the median ``better`` is 0;
  * hard: the centre spread reduced (--hard-spread) until thousands of identities come before
    the probe's own: what many marked identities cost.

The rank scan is the count pass plus 512 bytes of class ids per 64 KiB tile and one compare per
hit, so in the easy regime ``rank`` should cost ``labelled + count``; the line of ``rank`` carries
that sum, the margin (the yardsticks' own min-max spreads plus 10 %) and whether it is met.  The
hard regime has no bar.

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


def case(torch, dev, n, b, k, per_person, spread):
    """(G, identity labels of the rows, Q, identity labels of the probes)"""
    gen = torch.Generator(device=dev)
    gen.manual_seed(9876 + n + per_person)
    lab = (torch.arange(n, device=dev) // per_person).to(torch.int32)
    centres = spread * torch.randn((int(lab.max()) + 1, k), generator=gen, device=dev)
    G = (centres[lab.long()] + torch.randn((n, k), generator=gen, device=dev)).contiguous()
    plab = lab[torch.randint(0, n, (b,), generator=gen, device=dev)]
    Q = (centres[plab.long()] + torch.randn((b, k), generator=gen, device=dev)).contiguous()
    return G, lab, Q, plab.contiguous()


def thresholds(k, spread):
    """A range threshold between the within-identity scores (|a - b|^2 ~ 2 k, cosine ~ s^2 / (s^2 + 1))
    and the between-identity ones (~ 2 k (1 + s^2), ~ 0)."""
    within = spread * spread / (spread * spread + 1.0)
    return {"l2": 2.0 * k * (1.0 + 0.125 * min(spread * spread, 8.0)), "cosine": 0.6 * within}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--per-person", type=int, default=8)
    ap.add_argument("--easy-spread", type=float, default=4.0)
    ap.add_argument("--hard-spread", type=float, default=0.4, help="0 skips the hard regime")
    ap.add_argument("--metrics", default="l2,cosine")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("rank_timing.py: the median is taken over at least 5 repeats")
    sys.path.insert(0, os.path.join(ROOT, "face-detection-recognization-pca_amd"))

    import torch
    if not torch.cuda.is_available():
        sys.exit("rank_timing.py: no GPU (this tool measures; it has no CPU mode)")
    from eigenface import Engine
    from eigenface.evaluate import search_rank_plan
    from eigenface.neighbors import search_range_plan

    fh = open(args.out, "a") if args.out else None
    dev = torch.device("cuda", 0)
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    n, b, k = args.rows, args.probes, args.k
    for regime, spread in (("easy", args.easy_spread), ("hard", args.hard_spread)):
        if spread <= 0:
            continue
        G, lab, Q, plab = case(torch, dev, n, b, k, args.per_person, spread)
        eng.set_gallery(G)
        eng.set_gallery_labels(lab)
        classes = int(lab.max()) + 1
        words, per_piece, pieces = search_rank_plan(b, n, classes, eng.get_option("rank_bitmap_bytes"))
        chunks, tpi = search_range_plan(b, n, k)
        thr = thresholds(k, spread)
        for metric in args.metrics.split(","):
            t = thr[metric]
            better = torch.empty(b, dtype=torch.int32, device=dev)
            keys = torch.empty(b, dtype=torch.int64, device=dev)
            _, records, _ = eng.search_rank(Q, plab, None, metric, out=better)  # builds the class map, outside the timing
            records = records.clone()
            infos = {}

            def rank(metric=metric):
                infos["rank"] = eng.search_rank(Q, plab, None, metric, out=better)[2]

            def rank_given(metric=metric):
                infos["rank_given"] = eng.search_rank(Q, plab, None, metric, genuine=records, out=better)[2]

            def labelled(metric=metric):
                eng.search_labelled_keys(Q, plab, "same", None, metric, keys=keys)

            def count(metric=metric, t=t):
                infos["count"] = eng.search_range_counts(Q, t, metric)[1]

            res = timed(torch, {"rank": rank, "rank_given": rank_given, "labelled": labelled, "count": count},
                        args.warmup, args.repeats)
            bt = better.cpu().numpy()
            has = bt >= 0
            both = res["labelled"][0] + res["count"][0]
            margin = (res["labelled"][2] - res["labelled"][1]) + (res["count"][2] - res["count"][1]) + 0.1 * both
            for what, (med, lo, hi) in res.items():
                rec = {"regime": regime, "spread": spread, "rows": n, "probes": b, "k": k, "metric": metric,
                       "per_person": args.per_person, "classes": classes, "what": what, "ms": round(med, 3),
                       "min_ms": round(lo, 3), "max_ms": round(hi, 3), "repeats": args.repeats, "chunks": chunks,
                       "tiles_per_item": tpi, "pairs_per_s": round(n * b / (med * 1e-3), 1)}
                if what in ("rank", "rank_given"):
                    i = infos[what].cpu().numpy()
                    rec.update(fp64_pairs=int(i[0]), pieces=int(i[1]), words_per_probe=words,
                               bitmap_bytes=words * 4 * min(per_piece, (b + 255) // 256 * 256),
                               no_genuine=int((~has).sum()), median_better=float(np.median(bt[has])) if has.any() else None,
                               mean_better=round(float(bt[has].mean()), 2) if has.any() else None,
                               max_better=int(bt.max()), rank1=round(float((bt[has] == 0).mean()), 4) if has.any() else None)
                if what == "count":
                    i = infos[what].cpu().numpy()
                    rec.update(threshold=t, hits_per_probe=round(int(i[0]) / b, 2), fp64_pairs=int(i[1]))
                if what == "rank":
                    rec.update(yardsticks_ms=round(both, 3), margin_ms=round(margin, 3),
                               over_yardsticks_ms=round(med - both, 3))
                    if regime == "easy":
                        rec["within_bar"] = bool(med <= both + margin)
                if what == "rank_given":
                    rec["over_count_ms"] = round(med - res["count"][0], 3)
                emit(rec, fh)
        del G, lab, Q, plab
    eng.close()


if __name__ == "__main__":
    main()
