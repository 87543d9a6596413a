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

from . import _native as N
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


def label_one(person_name, similarity, threshold=0.7):
    """useless/scan.py:126-132, :205-213 for one model: ``(name, confidence, recognized)`` from the
    model's person name and its best cosine similarity; recognised on ``>=``.  A pure host function."""
    s = float(similarity)
    return person_name, s, bool(s >= threshold)


def label_pair(dark_name, dark_similarity, light_name, light_similarity, threshold=0.7):
    """``recognize_face_dual_model``'s rule (useless/scan.py:147-166): recognised when either
    model is (OR), the larger similarity, the dark model's name on ``>=``.  A pure host function."""
    _, ds, dr = label_one(dark_name, dark_similarity, threshold)
    _, ls, lr = label_one(light_name, light_similarity, threshold)
    return (dark_name if ds >= ls else light_name), max(ds, ls), dr or lr


def label_bank(bank, idx, sim, threshold=0.8, allowed=None):
    """``ModelBank.label`` in the Haar loop's record layout: ``[(name, confidence, recognized)]``,
    recognised where the winning model's row carries a label (person id other than -1)."""
    return [(name, conf, pid != -1) for pid, name, conf in bank.label(idx, sim, threshold, allowed)]


def _bank_layout(md, fallback_name):
    """A model dict as :class:`ModelBank` reads it.  A ``models/*_pca_model.pkl`` dict
    (``eigenfaces``, ``mean_face``, ``projected_data``, ``person_name``) gets its gallery under
    ``face_features``, one label for every row and its person name for that label."""
    if md is None or "face_features" in md or "projected_data" not in md:
        return md
    g = np.asarray(md["projected_data"])
    name = md.get("person_name", fallback_name)
    return {**md, "face_features": g, "face_labels": np.zeros(len(g), np.int64), "person_id_map": {name: 0}}


def _is_model(m):
    return isinstance(m, dict) and ("eigenfaces" in m or "pca" in m)


def _bank_resident(bank):
    """The shared engine holding ``bank``'s slots and, when the bank has a face gate, their
    reconstruction state: (re-)uploaded when someone else filled the engine's bank in between."""
    return bank._engine(reconstruction=bank.gate is not None)


class HaarScanner:
    """The Haar live loop (useless/scan.py:168-290, detection-v4.py:47-60: ``cvtColor`` ->
    ``detectMultiScale`` -> crop -> resize -> recognise) with one GPU call per frame
    (``ef_haar_scan_frame``): one upload of the frame, one download of the results, one
    synchronisation; the rectangles are grouped on the card.

    ``cascade``: a cascade dict (``haar.load_cascade``) or the path of OpenCV's XML.  ``models``:
    one model dict, a ``(dark, light)`` pair, or the ``{name: model}`` dict :class:`ModelBank`
    takes; both on-disk layouts are accepted (``face_model.pkl``, ``models/*_pca_model.pkl``).
    Faces are resized to ``int(sqrt(face_dimensions))`` squared (the models' pixel count).  At
    most ``max_faces`` rectangles of a frame are recognised, the first in OpenCV's order.  A
    frame with more than ``max_candidates`` ungrouped candidates goes through the separate calls
    (``CascadeClassifier.detect``, ``preprocess_rois``, the bank) instead, with the same result.
    ``face_gate`` is :class:`ModelBank`'s."""

    def __init__(self, cascade, models, frame_shape, device=0, scale_factor=1.1, min_neighbors=5, min_size=(30, 30),
                 max_size=(), max_faces=8, threshold=0.7, face_gate=None, max_candidates=4096):
        from .haar import CascadeClassifier, load_cascade
        self.device = device
        self.frame_shape = (int(frame_shape[0]), int(frame_shape[1]))
        self.scale_factor, self.min_neighbors = float(scale_factor), int(min_neighbors)
        self.min_size, self.max_size = tuple(min_size) if min_size else (), tuple(max_size) if max_size else ()
        self.max_faces, self.max_candidates, self.threshold = int(max_faces), int(max_candidates), float(threshold)
        self.cascade = load_cascade(cascade) if isinstance(cascade, str) else cascade
        if _is_model(models):
            self.mode, named = "one", {models.get("person_name", "person"): models}
        elif isinstance(models, (tuple, list)):
            if len(models) != 2:
                raise ValueError("a model pair is (dark, light)")
            self.mode, named = "pair", {"dark": models[0], "light": models[1]}
        else:
            self.mode, named = "bank", dict(models)
        self.model_names = []
        layout = {}
        for key, info in named.items():
            wrapped = isinstance(info, dict) and "model_data" in info
            md = _bank_layout(info["model_data"] if wrapped else info, key)
            layout[key] = {**info, "model_data": md} if wrapped else md
            self.model_names.append(md.get("person_name", key) if isinstance(md, dict) else key)
        self.bank = ModelBank(layout, device, face_gate)
        if not len(self.bank) or (self.mode != "bank" and len(self.bank) != len(named)):
            raise ValueError("HaarScanner needs usable models")
        eng = get_engine(device)
        d = eng.bank_info()[1]
        first = next(iter(named.values()))
        first = first["model_data"] if isinstance(first, dict) and "model_data" in first else first
        side = int(np.sqrt(first.get("face_dimensions", d))) if isinstance(first, dict) else int(np.sqrt(d))
        if side * side != d:
            raise ValueError(f"the models take {d} pixels, not a square face")
        self.face_size = (side, side)
        self.classifier = CascadeClassifier(cascade=self.cascade, device=device)

    def _prepare(self):
        """The cascade, the plan and the bank's slots, (re-)uploaded when someone else used the
        shared engine's cascade or bank in between."""
        eng = get_engine(self.device)
        if getattr(eng, "haar_scan_owner", None) is not self or getattr(eng, "_haar_scan", None) is None:
            self.classifier.set_cascade(self.cascade)
            eng.haar_scan_prepare(self.frame_shape, self.scale_factor, self.min_neighbors, self.min_size, self.max_size,
                                  self.face_size, self.max_faces, self.max_candidates)
            eng.haar_scan_owner = self
        return _bank_resident(self.bank)

    def _separate_calls(self, eng, frame, rgb):
        """The frame through the calls ef_haar_scan_frame fuses, in its result layout."""
        f = frame.cpu().numpy() if hasattr(frame, "cpu") else np.asarray(frame)
        H, W = self.frame_shape
        gray = f if f.ndim == 2 else eng.preprocess([np.ascontiguousarray(f)], (W, H), rgb=rgb)[0].reshape(H, W)
        found, cand = self.classifier.detect(gray, self.scale_factor, self.min_neighbors, self.min_size, self.max_size,
                                             return_candidates=True)
        F = self.max_faces
        rects = np.zeros((F, 4), np.int32)
        rects[:min(len(found), F)] = found[:F]
        rows = np.zeros((F, self.face_size[0] * self.face_size[1]), np.uint8)
        if len(found):
            rows[:min(len(found), F)] = eng.preprocess_rois(gray, found[:F], self.face_size)
        head = np.zeros(1, dtype=N.HAAR_SCAN_HEAD_DTYPE)[0]
        head["status"], head["n_candidates"] = N.EF_HAAR_SCAN_OVERFLOW, len(cand)
        head["n_rects"], head["n_faces"] = len(found), min(len(found), F)
        if self.bank.gate is None:
            keys, _, best, _ = eng.bank_recognize_raw(rows, "cosine")
            return head, rects, keys, best, rows
        keys, _, best, _, eps, en = eng.bank_recognize_gated_raw(rows, self.bank.gate, "cosine", relative=True)
        return head, rects, keys, best, rows, eps, en

    def scan_raw(self, frame, rgb=False):
        """``Engine.haar_scan_frame`` on this scanner's plan: (head, rects, keys, best_slot, rows)
        and, with a face gate, (dffs2, energy).  A frame whose candidates overflow the plan comes
        from the separate calls, as NumPy arrays, with EF_HAAR_SCAN_OVERFLOW left in head."""
        eng = self._prepare()
        out = eng.haar_scan_frame(frame, "cosine", gate=self.bank.gate, relative=True, rgb=rgb)
        status = int(out[0][0]) if hasattr(out[0], "cpu") else int(out[0]["status"])
        if status & N.EF_HAAR_SCAN_OVERFLOW:
            out = self._separate_calls(eng, frame, rgb)
        return out

    def scan(self, frame, rgb=False):
        """The reference's list ``[(x, y, w, h, name, confidence, recognized)]`` for one frame:
        :func:`label_one` for one model, :func:`label_pair` for a pair, :func:`label_bank` for a
        bank, on the similarities the bank call returned."""
        out = [t.cpu().numpy() if hasattr(t, "cpu") else t for t in self.scan_raw(frame, rgb)]
        head, rects, keys = out[0], out[1], out[2]
        nf = int(head[3]) if isinstance(head, np.ndarray) and head.dtype.names is None else int(head["n_faces"])
        if nf == 0:
            return []
        k = np.ascontiguousarray(keys[:nf])
        idx, sim = decode_keys(k.reshape(-1), "cosine")
        idx, sim = idx.reshape(k.shape), sim.reshape(k.shape)
        if self.mode == "one":
            labels = [label_one(self.model_names[0], s[0], self.threshold) for s in sim]
        elif self.mode == "pair":
            labels = [label_pair(self.model_names[0], s[0], self.model_names[1], s[1], self.threshold) for s in sim]
        else:
            allowed = face_gate_mask(out[5][:nf], out[6][:nf], self.bank.gate) if len(out) > 5 else None
            labels = label_bank(self.bank, idx, sim, self.threshold, allowed)
        return [(int(x), int(y), int(w), int(h), *lab) for (x, y, w, h), lab in zip(rects[:nf], labels)]


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
        return _bank_resident(self.bank)

    def scan_raw(self, frame, rgb=False):
        """``Engine.scan_frame`` on this scanner's plan: (dets, keys, best_slot, rows); with a
        face gate ``Engine.scan_frame_gated``: the same and (dffs2, energy)."""
        eng = self._prepare()
        if self.bank.gate is None:
            return eng.scan_frame(frame, "cosine", rgb=rgb)
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
