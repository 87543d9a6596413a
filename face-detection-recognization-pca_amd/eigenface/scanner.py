"""Frame scanner: the live loop of scan-template-v4.py (``process_live_camera``, :340-422) with
one GPU call per frame.

Per frame the reference converts BGR to grey, runs ``template_match_all_models``, crops every
detection out of the frame, greys and resizes it to 64 x 64 and runs
``recognize_face_all_models`` on it, then applies a selection rule (:351-377) and a decision rule
(:393-401).  :class:`FrameScanner` keeps every person's templates (``TemplateLocaliser``) and
models (``ModelBank``) resident and sends a frame through all of it with one ``ef_scan_frame``
call: one upload of the frame, one download of the results, one synchronisation.  The selection
and decision rules are host logic on a handful of numbers: :func:`decide`.

No camera, video or drawing here: frames come in as arrays, records go out as dicts.
"""
from __future__ import annotations

import numpy as np

from .bank import ModelBank, face_gate_mask
from .engine import decode_keys
from .image import SCALES, TemplateLocaliser
from .pca import get_engine

FACE_SIZE = (64, 64)  # scan-template-v4.py:261


def decide(detections, pca_results):
    """scan-template-v4.py:351-401 on the detections of one frame (the dicts of
    ``template_match_all_models``) and their ``(person_id, name, confidence)`` tuples of
    ``recognize_face_all_models``: the reference's result records (:413-420) without
    ``frame_number``.  A pure host function.

    * More than one detection: only the one maximising
      ``min(w * h / 40000, 1) * 0.5 + pca_confidence * 0.5`` is kept, under a strict ``>`` from
      -1 (the first of equal scores).
    * The name is the template's if the PCA name equals it or ``pca_confidence < 0.5``, else the
      PCA name; ``final_confidence`` follows the same branch.
    * The name is "unknown" if ``pca_confidence < 0.8 or template_confidence < 0.7``."""
    pairs = list(zip(detections, pca_results))
    if len(pairs) > 1:
        best, best_score = None, -1
        for det, res in pairs:
            size = det["width"] * det["height"]
            combined = min(size / (200 * 200), 1.0) * 0.5 + res[2] * 0.5
            if combined > best_score:
                best_score = combined
                best = (det, res)
        pairs = [best] if best else []
    records = []
    for det, (_, pca_name, pca_conf) in pairs:
        person, template_conf = det["person_name"], det["confidence"]
        if pca_name == person or pca_conf < 0.5:
            final_name, final_conf = person, template_conf
        else:
            final_name, final_conf = pca_name, pca_conf
        if pca_conf < 0.8 or template_conf < 0.7:
            final_name = "unknown"
        records.append({"person_name": final_name, "template_confidence": template_conf,
                        "pca_confidence": pca_conf, "final_confidence": final_conf,
                        "x": det["x"], "y": det["y"], "width": det["width"], "height": det["height"]})
    return records


def corner_integers(frame_width, frame_height, corner_threshold=0.15, border_threshold=0.05):
    """(corner_w, corner_h, border_w, border_h) of is_detection_in_corner
    (scan-template-v4.py:75-125), as ef_scan_prepare computes them once per plan."""
    return (int(frame_width * corner_threshold), int(frame_height * corner_threshold),
            int(frame_width * border_threshold), int(frame_height * border_threshold))


class FrameScanner:
    """The reference's models (the dict ``load_all_models`` fills: per person ``template_images``,
    its first five detection faces as ``{"image": grey uint8, ...}`` or plain arrays, and
    ``model_data``) prepared for frames of ``frame_shape`` (H, W[, channels]).

    A person without templates (or whose ``detection_data`` is present and empty, :146) is
    never detected; a person whose ``model_data`` is None or unusable has no slot in the bank,
    as in :class:`ModelBank`.  At least one usable model is required.

    ``face_gate`` is :class:`ModelBank`'s: with it the frame goes through ``ef_scan_frame_gated``,
    and a detection whose crop no model accepts as a face reaches :func:`decide` as
    ``(-1, "unknown", 0.0)``."""

    def __init__(self, models, frame_shape, device=0, threshold=0.6, recognize_threshold=0.8, scales=SCALES,
                 face_gate=None):
        self.device = device
        self.models = models
        self.frame_shape = (int(frame_shape[0]), int(frame_shape[1]))
        self.threshold = float(threshold)
        self.recognize_threshold = float(recognize_threshold)
        templates = {}
        for person, info in models.items():
            imgs = []
            if info.get("detection_data", True):
                imgs = [t["image"] if isinstance(t, dict) else t for t in info.get("template_images") or []]
            templates[person] = imgs
        self.localiser = TemplateLocaliser(templates, self.frame_shape, scales, device)
        self.persons = self.localiser.persons
        group = {p: g for g, p in enumerate(self.persons)}
        self.prob_group = np.array([group[m[0]] for m in self.localiser.meta], np.int32)
        self.bank = ModelBank(models, device, face_gate)
        if not len(self.bank):
            raise ValueError("FrameScanner needs at least one usable model")

    def _prepare(self):
        """The localiser's operands, the scan plan and the bank's slots, (re-)uploaded when
        someone else used the shared engine's localiser or bank in between."""
        eng = get_engine(self.device)
        if getattr(eng, "scan_owner", None) is not self or getattr(eng, "_scan", None) is None:
            self.localiser._prepared = False
            self.localiser._prepare()
            eng.scan_prepare(self.prob_group, max(len(self.persons), 1), FACE_SIZE, self.threshold)
            eng.scan_owner = self
        if getattr(eng, "bank_owner", None) is not self.bank:
            self.bank.refresh()
        return eng

    def scan_raw(self, frame, rgb=False):
        """``Engine.scan_frame`` on this scanner's plan: (dets, keys, best_slot, rows); with a
        face gate ``Engine.scan_frame_gated``: the same and (dffs2, energy)."""
        eng = self._prepare()
        if self.bank.gate is None:
            return eng.scan_frame(frame, "cosine", rgb=rgb)
        if not self.bank._recon_up:
            self.bank._upload_reconstruction(eng)
        return eng.scan_frame_gated(frame, self.bank.gate, "cosine", relative=True, rgb=rgb)

    def scan(self, frame, rgb=False):
        """(detections, pca_results) of one BGR (or grey) frame: the dicts of
        ``template_match_all_models`` (:176-184) in model order, and per detection the
        ``(person_id, name, confidence)`` of ``recognize_face_all_models`` on its crop."""
        dets, keys, _, _, *gate_out = self.scan_raw(frame, rgb)
        found = np.flatnonzero(dets["found"])
        detections = []
        for g in found:
            d = dets[g]
            detections.append({"x": int(d["x"]), "y": int(d["y"]), "width": int(d["w"]), "height": int(d["h"]),
                               "person_name": self.persons[g], "confidence": float(d["confidence"]),
                               "scale": self.localiser.meta[int(d["problem"])][1]})
        if not len(found):
            return detections, []
        k = np.ascontiguousarray(keys[found])
        idx, sim = decode_keys(k.reshape(-1), "cosine")
        allowed = face_gate_mask(gate_out[0][found], gate_out[1][found], self.bank.gate) if gate_out else None
        return detections, self.bank.label(idx.reshape(k.shape), sim.reshape(k.shape), self.recognize_threshold, allowed)

    decide = staticmethod(decide)

    def scan_frame(self, frame, rgb=False):
        """The reference's result records of one frame (without ``frame_number``)."""
        return decide(*self.scan(frame, rgb))

    def process_frames(self, frames, rgb=False):
        """The records of a sequence of frames, each with its ``frame_number`` (:413-420)."""
        for n, frame in enumerate(frames):
            for rec in self.scan_frame(frame, rgb):
                yield {"frame_number": n, **rec}
