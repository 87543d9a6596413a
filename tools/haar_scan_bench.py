#!/usr/bin/env python3
"""Haar route in one call against the sequence of separate calls (DESIGN.md "K12s Haar scan").

Workload: the Haar bench's 640 x 480 frame as a BGR frame (bench.haar_bench; blue lifted and red
lowered so the channels differ), its synthetic 25-stage / 2913-stump cascade, detectMultiScale(1.1,
5, (30, 30)), a 4-slot model bank of 64 x 64 models with 32 components, max_faces = 8.  The frame
holds no face: ~260k windows pass stage 0, none passes all stages, so the rectangle list is empty.

  separate          what a caller had to do before ef_haar_scan_frame, with the same answer (the
                    arrays HaarScanner.scan_raw returns): grey on the host, CascadeClassifier.detect
                    (upload, kernels, two host reads of counters, download, host grouping),
                    preprocess_rois of the rectangles (skipped when there are none) and
                    bank_recognize of the max_faces rows (upload, kernels, download)
  separate_pregrey  the same from a frame greyed beforehand
  detect_pregrey    CascadeClassifier.detect alone on the greyed frame: what a caller who skips the
                    bank on a frame without rectangles pays
  scan              HaarScanner.scan_raw: one ef_haar_scan_frame in host form (one upload, one
                    download, one synchronisation)

The host grey is a NumPy integer expression here (OpenCV is not a dependency); cv2.cvtColor is far
cheaper, which is why the pre-greyed legs exist.  All legs are wall time per frame,
synchronisation included.  Protocol: 2 warm-ups of each leg, then the legs alternated, 5 repeats
of 200 frames each; the median repeat and the min-max spread of each leg are recorded.  A further
pass with the device timers on records EF_KERNEL_HAAR_SCAN of the scan next to EF_KERNEL_HAAR of
ef_haar_detect on the same frame (and the separate legs' ingest and bank timers).

  python tools/haar_scan_bench.py [--out profiles/haar_scan.json] [--repeats 5] [--frames 200]
  python tools/haar_scan_bench.py --keep 0.66 --max-candidates 16384   # more survivors per stage
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
sys.path.insert(0, ROOT)

H, W = 480, 640
FACE = 64
SLOTS = 4
MAX_FACES = 8


def bgr2gray_host(img):
    a = img.astype(np.int32)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def workload(keep=0.6):
    """(BGR frame, cascade, models): the Haar bench's frame and cascade (the cascade is
    calibrated on the frame's own grey plane so that the share `keep` of the windows reaching a
    stage passes it; 0.6 is the Haar bench's) and SLOTS models in the *_pca_model.pkl layout."""
    import bench
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    f = 100 + 50 * np.sin(xx / 23.0) * np.cos(yy / 31.0) + rng.normal(0, 12, (H, W))
    g = np.clip(np.rint(f), 0, 255).astype(np.int32)
    frame = np.stack([np.clip(g + 9, 0, 255), g, np.clip(g - 12, 0, 255)], -1).astype(np.uint8)
    cascade = bench.synth_frontal_cascade(bgr2gray_host(frame), keep=keep)
    models = {}
    d, k = FACE * FACE, 32
    for s in range(SLOTS):
        x = rng.integers(0, 256, (k, d)).astype(np.float64)
        mean = x.mean(0)
        _, _, vt = np.linalg.svd(x - mean, full_matrices=False)
        eig = np.ascontiguousarray(vt.T, dtype=np.float32)
        mean = mean.astype(np.float32)
        models[f"person{s}"] = {"eigenfaces": eig, "mean_face": mean, "person_name": f"person{s}",
                                "projected_data": ((x.astype(np.float32) - mean) @ eig).astype(np.float32),
                                "face_dimensions": d}
    return frame, cascade, models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--keep", type=float, default=0.6,
                    help="share of windows passing each stage of the synthetic cascade (0.6: no window passes all 25; "
                         "higher values leave candidates for the grouping, the ROI rows and the bank)")
    ap.add_argument("--max-candidates", type=int, default=4096)
    a = ap.parse_args()

    from eigenface import HaarScanner, get_engine
    eng = get_engine(0)  # fails without a GPU: there is nothing to measure elsewhere
    frame, cascade, models = workload(a.keep)
    sc = HaarScanner(cascade, models, (H, W), max_faces=MAX_FACES, max_candidates=a.max_candidates)
    grey0 = bgr2gray_host(frame)

    def separate(grey=None):
        # the scanner's own fallback: the calls ef_haar_scan_frame fuses, in its result layout
        return sc._separate_calls(eng, bgr2gray_host(frame) if grey is None else grey, False)

    def separate_pregrey():
        return separate(grey0)

    def detect_pregrey():
        return sc.classifier.detect(grey0, sc.scale_factor, sc.min_neighbors, sc.min_size, sc.max_size)

    def scan():
        return sc.scan_raw(frame)

    # the legs answer alike, bit for bit (the status word apart: the fallback leaves its mark there)
    s1 = scan()
    s0 = separate()
    assert int(s1[0]["status"]) == 0, s1[0]
    assert tuple(s0[0])[1:] == tuple(s1[0])[1:], (s0[0], s1[0])
    for x, y in zip(s0[1:], s1[1:]):
        np.testing.assert_array_equal(x, y)
    layers, visitable, _, max_cand = eng.haar_scan_info()

    def run(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) / n * 1e3

    legs = {"separate": separate, "separate_pregrey": separate_pregrey, "detect_pregrey": detect_pregrey,
            "scan": scan, "host_grey_alone": lambda: bgr2gray_host(frame)}
    for _ in range(2):  # warm-ups
        for fn in legs.values():
            run(fn, a.frames)
    wall = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            wall[name].append(run(fn, a.frames))

    eng.timing(True)
    dev = {}
    for name, fn, timers in (("separate_pregrey", separate_pregrey, ("haar", "ingest", "project", "search")),
                             ("detect_pregrey", detect_pregrey, ("haar",)),
                             ("scan", scan, ("haar_scan", "project", "search"))):
        fn()
        eng.timing_reset()
        run(fn, a.frames)
        dev[name] = {t: eng.timing_get(t)[0] / a.frames for t in timers}
    eng.timing(False)
    eng.timing_reset()

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
                "spread_ms": float(max(v) - min(v)), "repeats_ms": [float(x) for x in v]}

    st = {name: stats(v) for name, v in wall.items()}
    pre, scn = st["separate_pregrey"], st["scan"]
    spread = max(pre["spread_ms"], scn["spread_ms"])
    # the scan's span holds the grey plane, the detector, the grouping, the ROI rows and the bank;
    # the bank's two kernels are timed inside it as well, so the detector's share is what is left
    scan_detect = dev["scan"]["haar_scan"] - dev["scan"]["project"] - dev["scan"]["search"]
    rec = {
        "workload": {"frame": [H, W, 3], "cascade_stages": len(cascade["stages"]),
                     "cascade_stumps": sum(len(s[1]) for s in cascade["stages"]), "cascade_keep": a.keep,
                     "bank_slots": SLOTS,
                     "face": [FACE, FACE], "max_faces": MAX_FACES, "max_candidates": max_cand,
                     "pyramid_layers": layers, "visitable_windows": visitable,
                     "candidates": int(s1[0]["n_candidates"]), "rectangles": int(s1[0]["n_rects"])},
        "protocol": {"warmups": 2, "repeats": a.repeats, "frames_per_repeat": a.frames, "alternated": True},
        "wall_ms_per_frame": st,
        "device_ms_per_frame": dev,
        "acceptance": {
            "wall_margin_ms": pre["median_ms"] - scn["median_ms"],
            "larger_spread_ms": spread,
            "wall_met": bool(pre["median_ms"] - scn["median_ms"] > spread),
            "wall_margin_vs_detect_alone_ms": st["detect_pregrey"]["median_ms"] - scn["median_ms"],
            "device_scan_span_ms": dev["scan"]["haar_scan"],
            "device_scan_span_without_bank_ms": scan_detect,
            "device_detect_ms": dev["detect_pregrey"]["haar"],
            "device_excess_ms": scan_detect - dev["detect_pregrey"]["haar"],
        },
    }
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
