#!/usr/bin/env python3
"""Frame scan against the sequence of separate calls (DESIGN.md "K14 frame scan").

Workload: one 640 x 480 BGR frame, 4 persons x 5 templates x 3 scales (60 localiser problems),
a 4-slot model bank of 64 x 64 models.  Two ways of answering the live loop's question for it:

  sequence  what a caller had to do before ef_scan_frame: grey on the host,
            TemplateLocaliser.template_match_all_models (upload, kernels, download, the rule in
            Python), the crops cut out of the frame on the host, ModelBank.recognize_faces
            (upload, ingest kernel, download, upload, bank kernels, download)
  scan      FrameScanner.scan: one ef_scan_frame call in host form (one upload, one download,
            one synchronisation) and the same labelling in Python

The sequence's host grey is a NumPy integer expression here (OpenCV is not a dependency); the
reference's cv2.cvtColor is far cheaper.  So the grey is also timed alone, and a third leg,
"sequence_pregrey", runs the sequence from a frame greyed beforehand: what a caller whose grey
costs nothing would compare the scan with.

All legs are wall time per frame, synchronisation included.  Protocol: 2 warm-ups of each leg, then
the legs alternated, 5 repeats of 200 frames each; the median repeat and the min-max spread of
each leg are recorded.  A further pass with the device timers on records EF_KERNEL_SCAN next to
the sum of EF_KERNEL_TMATCH, EF_KERNEL_INGEST and the bank's two timers over the sequence.

  python tools/scan_frame_bench.py [--out FILE] [--repeats 5] [--frames 200]
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

H, W = 480, 640
PERSONS = ["ana", "ben", "cho", "dev"]
# top-left corners of the five templates of each person (away from the corner / border zones)
# and their sizes: the persons' faces differ in size, as the selection rule expects
SPOTS = {"ana": ((200, 150), (96, 96)), "ben": ((380, 120), (80, 88)), "cho": ((150, 300), (110, 100)),
         "dev": ((420, 310), (72, 72))}


def bgr2gray_host(img):
    a = img.astype(np.int32)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def workload(seed=0):
    """(frame, models): the first template of three persons is cut from the frame's grey, the
    others (and all of the fourth person's) are noise, so three persons are found."""
    from eigenface.compat import FaceTrainer
    from eigenface.synth import mean_face
    rng = np.random.default_rng(seed)
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    grey = bgr2gray_host(frame)
    models = {}
    for i, p in enumerate(PERSONS):
        (x, y), (tw, th) = SPOTS[p]
        templates = [rng.integers(0, 256, (th, tw), dtype=np.uint8) for _ in range(5)]
        if p != "dev":
            templates[0] = grey[y:y + th, x:x + tw].copy()
        base = mean_face(64).reshape(-1)
        faces = np.clip(base[None, :] + rng.normal(0, 30, (64, 4096)) + rng.normal(0, 20, (64, 1)), 0, 255)
        tr = FaceTrainer()
        tr.face_images = faces.astype(np.uint8)
        tr.face_info = [{"face_id": j} for j in range(len(faces))]
        tr.assign_labels_interactive(p)
        if not tr.train_pca_model():
            raise RuntimeError(f"training the model of {p} failed")
        models[p] = {"model_data": tr.model_dict(), "template_images": [{"image": t} for t in templates],
                     "detection_data": {"faces": [{}]}}
    return frame, models


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the JSON record here as well")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200)
    a = ap.parse_args()

    from eigenface import FrameScanner, get_engine
    eng = get_engine(0)  # fails without a GPU: there is nothing to measure elsewhere
    frame, models = workload()
    sc = FrameScanner(models, (H, W))

    grey0 = bgr2gray_host(frame)

    def sequence(grey=None):
        if grey is None:
            grey = bgr2gray_host(frame)
        dets = sc.localiser.template_match_all_models(grey, sc.threshold)
        crops = [frame[d["y"]:d["y"] + d["height"], d["x"]:d["x"] + d["width"]] for d in dets]
        return dets, sc.bank.recognize_faces(crops, sc.recognize_threshold)

    def sequence_pregrey():
        return sequence(grey0)

    def scan():
        return sc.scan(frame)

    # the two legs answer alike: same detections, same names (confidences within the two
    # projections' rounding: the bank's K-split depends on the batch size)
    d1, p1 = scan()
    d0, p0 = sequence()
    assert [(d["person_name"], d["x"], d["y"], d["width"], d["height"], d["confidence"]) for d in d0] == \
           [(d["person_name"], d["x"], d["y"], d["width"], d["height"], d["confidence"]) for d in d1], (d0, d1)
    assert [r[:2] for r in p0] == [r[:2] for r in p1] and len(d1) == 3, (p0, p1)

    def run(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) / n * 1e3

    legs = {"sequence": sequence, "sequence_pregrey": sequence_pregrey, "scan": scan,
            "host_grey_alone": lambda: bgr2gray_host(frame)}
    for _ in range(2):  # warm-ups
        for fn in legs.values():
            run(fn, a.frames)
    wall = {name: [] for name in legs}
    for _ in range(a.repeats):
        for name, fn in legs.items():
            wall[name].append(run(fn, a.frames))

    eng.timing(True)
    dev = {}
    for name, fn, timers in (("sequence", sequence, ("tmatch", "ingest", "project", "search")),
                             ("scan", scan, ("scan",))):
        eng.timing_reset()
        run(fn, a.frames)
        dev[name] = {t: eng.timing_get(t)[0] / a.frames for t in timers}
        dev[name]["total"] = sum(dev[name].values())
    eng.timing(False)
    eng.timing_reset()

    def stats(v):
        return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
                "spread_ms": float(max(v) - min(v)), "repeats_ms": [float(x) for x in v]}

    seq, scn, pre = stats(wall["sequence"]), stats(wall["scan"]), stats(wall["sequence_pregrey"])
    rec = {
        "workload": {"frame": [H, W, 3], "persons": len(PERSONS), "templates_per_person": 5, "scales": 3,
                     "problems": len(sc.localiser.problems), "bank_slots": len(sc.bank), "detections": len(d1)},
        "protocol": {"warmups": 2, "repeats": a.repeats, "frames_per_repeat": a.frames, "alternated": True},
        "wall_ms_per_frame": {"sequence": seq, "sequence_pregrey": pre, "scan": scn,
                              "host_grey_alone": stats(wall["host_grey_alone"])},
        "device_ms_per_frame": dev,
        "acceptance": {
            "wall_margin_ms": seq["median_ms"] - scn["median_ms"],
            "wall_met": bool(seq["median_ms"] - scn["median_ms"] > seq["spread_ms"]),
            "wall_margin_pregrey_ms": pre["median_ms"] - scn["median_ms"],
            "wall_met_pregrey": bool(pre["median_ms"] - scn["median_ms"] > pre["spread_ms"]),
            "device_excess_ms": dev["scan"]["total"] - dev["sequence"]["total"],
            "device_met": bool(dev["scan"]["total"] - dev["sequence"]["total"] <= seq["spread_ms"]),
        },
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
