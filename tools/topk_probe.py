#!/usr/bin/env python3
"""Cost of the top-m search at the benchmark shapes, on one GPU.

Times Engine.search_topk_keys on device tensors for m in {1, 10, 64} at the C3 shape
(1M x 128, 4096 probes) and the C5 shape (1M x 512), under the L2 fp32 and split-bf16 scans,
next to

  * Engine.search_keys with the prefix scan off (one plain top-1 scan, the unit the ratios
    are in) — with --top1-only this is all the tool runs, and --pkg points it at another
    checkout's package, so the parent commit is timed by the same code;
  * what a user writes without the library: chunked fp32 Q @ G.T, torch.topk per chunk and a
    merge of the chunk lists.

Every figure is device time from events on the launch stream around K back-to-back calls,
the median of R repeats after warm-up, the variants of one shape interleaved inside each
repeat.  --check compares the rows of a 256-probe subset with fp64 GEMMs on the GPU
(parity_util.top2_device's scores, extended to rank m).  One JSON line per measurement goes
to stdout and, with --out, to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = {"c3": 128, "c5": 512}
WINDOW = 1e-12


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def timed(torch, fns, steps, warmup, repeats):
    """{name: median ms per call}: the variants run interleaved inside every repeat."""
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


def torch_topk_fp32(torch, Q, G, gg, m, chunk=131072):
    """The hand-written route: fp32 distances chunk by chunk, topk per chunk, merge."""
    qq = (Q * Q).sum(1, keepdim=True)
    vals, rows = [], []
    for a in range(0, G.shape[0], chunk):
        s = torch.addmm(gg[a:a + chunk][None, :] + qq, Q, G[a:a + chunk].T, alpha=-2.0)
        v, i = torch.topk(s, min(m, s.shape[1]), dim=1, largest=False)
        vals.append(v)
        rows.append(i + a)
    v, r = torch.cat(vals, 1), torch.cat(rows, 1)
    v, j = torch.topk(v, min(m, v.shape[1]), dim=1, largest=False)
    return torch.gather(r, 1, j), v


def fp64_reference(torch, q, G, m, chunk=131072):
    """(scores, rows) of the m + 1 smallest fp64 squared distances per probe (expanded form)."""
    q64 = q.double()
    qq = (q64 * q64).sum(1)
    bv = torch.full((q.shape[0], 0), 0.0, dtype=torch.float64, device=q.device)
    br = torch.zeros((q.shape[0], 0), dtype=torch.int64, device=q.device)
    for a in range(0, G.shape[0], chunk):
        g64 = G[a:a + chunk].double()
        s = qq[:, None] + (g64 * g64).sum(1)[None, :] - 2.0 * (q64 @ g64.T)
        v, i = torch.topk(s, min(m + 1, s.shape[1]), dim=1, largest=False)
        bv, br = torch.cat([bv, v], 1), torch.cat([br, i + a], 1)
        v, j = torch.topk(bv, min(m + 1, bv.shape[1]), dim=1, largest=False)
        bv, br = v, torch.gather(br, 1, j)
        del s
    return bv, br


def check_rows(torch, q, G, gmax2, rows, m):
    """Rows (b, m) against the fp64 reference: every rank's score inside the tie window of the
    reference's, and the same row wherever the reference's neighbours are clear of it."""
    bv, br = fp64_reference(torch, q, G, m)
    q64 = q.double()
    scale = (q64 * q64).sum(1) + gmax2
    mine = ((q64[:, None, :] - G[rows].double()) ** 2).sum(-1)
    w = 1.1 * WINDOW * (bv[:, :m].abs() + scale[:, None])
    inside = ((mine - bv[:, :m]).abs() <= w)
    lo = torch.cat([torch.full_like(bv[:, :1], -float("inf")), bv[:, :m - 1]], 1)
    clear = ((bv[:, :m] - lo) > w) & ((bv[:, 1:m + 1] - bv[:, :m]) > w)
    same = rows == br[:, :m]
    distinct = bool((torch.sort(rows, 1).values.diff(dim=1) != 0).all())
    return {"ranks": int(rows.numel()), "inside_window": int(inside.sum()), "clear": int(clear.sum()),
            "clear_and_equal": int((clear & same).sum()), "distinct": distinct,
            "ok": bool(inside.all() and (same | ~clear).all() and distinct)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="c3,c5")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--probes", type=int, default=4096)
    ap.add_argument("--ms", default="1,10,64", help="the m values")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--top1-only", action="store_true", help="time search_keys only (works on older checkouts)")
    ap.add_argument("--no-torch-baseline", action="store_true")
    ap.add_argument("--check", action="store_true", help="fp64 check of a 256-probe subset")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "face-detection-recognization-pca_amd"),
                    help="directory holding the eigenface package to measure")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))

    import torch
    if not torch.cuda.is_available():
        sys.exit("topk_probe.py: no GPU (this tool measures; it has no CPU mode)")
    from eigenface import Engine, synth

    fh = open(args.out, "a") if args.out else None
    dev = torch.device("cuda", 0)
    ms = [int(v) for v in args.ms.split(",")]
    eng = Engine(0)
    eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    eng.set_option("search_prefix", 0)
    for shape in args.shapes.split(","):
        k = SHAPES[shape]
        t0 = time.perf_counter()
        G = synth.gallery_rows(0, args.rows, k)
        targets = np.random.default_rng(2024).integers(0, args.rows, args.probes)
        rng = np.random.default_rng(5)
        Q = (G[targets] + 0.05 * rng.standard_normal((args.probes, k)).astype(np.float32) * synth.spectrum(k).astype(np.float32))
        Gd, Qd = torch.from_numpy(G).to(dev), torch.from_numpy(Q).to(dev)
        eng.set_gallery(Gd)
        gg = (Gd * Gd).sum(1)
        gmax2 = float(gg.double().max())
        keys1 = torch.empty(args.probes, dtype=torch.int64, device=dev)
        base = {"label": args.label, "shape": shape, "rows": args.rows, "k": k, "probes": args.probes,
                "steps": args.steps, "repeats": args.repeats}
        emit({**base, "what": "setup_s", "value": round(time.perf_counter() - t0, 1)}, fh)
        for scan, name in ((0, "fp32"), (1, "split")):
            eng.set_option("search_split_bf16", scan)
            fns = {"top1": lambda: eng.search_keys(Qd, "l2", keys=keys1)}
            outs = {}
            if not args.top1_only:
                for m in ms:
                    outs[m] = torch.empty((args.probes, m), dtype=torch.int64, device=dev)
                    fns[f"topk_m{m}"] = (lambda m=m: eng.search_topk_keys(Qd, m, "l2", keys=outs[m]))
            res = timed(torch, fns, args.steps, args.warmup, args.repeats)
            t1 = res["top1"][0]
            for what, (med, lo, hi) in res.items():
                rec = {**base, "scan": name, "what": what, "ms": round(med, 4), "min_ms": round(lo, 4),
                       "max_ms": round(hi, 4), "top1_scans": round(med / t1, 3)}
                if what.startswith("topk"):
                    m = int(what.split("m")[1])
                    eng.search_topk_keys(Qd, m, "l2", keys=outs[m])
                    rec["topk_stats"] = list(eng.topk_stats())
                    rec["rank0_equals_top1"] = bool((outs[m][:, 0] == eng.search_keys(Qd, "l2")).all())
                    if args.check:
                        sub = slice(0, 256)
                        rows = (outs[m][sub] & 0xFFFFFFFF)
                        rec["check256"] = check_rows(torch, Qd[sub], Gd, gmax2, rows, m)
                emit(rec, fh)
        if not args.top1_only and not args.no_torch_baseline:
            fns = {f"torch_topk_m{m}": (lambda m=m: torch_topk_fp32(torch, Qd, Gd, gg, m)) for m in ms}
            for what, (med, lo, hi) in timed(torch, fns, max(1, args.steps // 5), 1, min(3, args.repeats)).items():
                emit({**base, "scan": "torch fp32 GEMM + topk", "what": what, "ms": round(med, 4),
                      "min_ms": round(lo, 4), "max_ms": round(hi, 4)}, fh)
        del Gd, Qd, gg
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
