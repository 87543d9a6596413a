"""Model bank: every per-person model of the scanner resident on the GPU at once.

``MultiModelFaceScanner.recognize_face_all_models`` (scan-template-v4.py:289-319) loops over
the per-person models for every face: each has its own scaler + PCA and its own small gallery,
and the best cosine similarity is kept under a strict ``>``.  :class:`ModelBank` uploads all of
them once (``Engine.bank_add``) and answers a batch of faces with one ``ef_bank_recognize``
call, whose launch count does not depend on the number of models.
"""
from __future__ import annotations

import numpy as np

from .compat import _folded, preprocess_faces
from .pca import get_engine


def best_over_models(scores, metric="cosine"):
    """The reference's choice over models (scan-template-v4.py:293-309) for a table
    ``scores[b, M]`` of per-model best scores: walk the models in order, a model wins only
    with a strictly greater value than the best so far.  Cosine: the value is the similarity
    and the walk starts from 0.0, so nothing wins without a similarity > 0.  L2: the value is
    the negated distance and the walk starts from -inf, so the first smallest distance wins.
    NaN (an empty gallery) never wins.  Returns int32 slots, -1 where no model wins."""
    s = np.asarray(scores, dtype=np.float32)
    if s.ndim != 2:
        raise ValueError("scores must be (b, M)")
    l2 = str(metric).lower() == "l2"
    out = np.full(s.shape[0], -1, np.int32)
    for p in range(s.shape[0]):
        best = np.float32(-np.inf) if l2 else np.float32(0.0)
        for m in range(s.shape[1]):
            v = -s[p, m] if l2 else s[p, m]
            if v > best:  # False for NaN
                best = v
                out[p] = m
    return out


class ModelBank:
    """The scanner's models (the dict ``load_all_models`` returns, or ``{name: model_data}``)
    as one resident bank.  A model that is ``None`` is left out silently and one that fails
    to fold or upload is reported with the reference's ``Error recognizing with model
    {name}: {e}`` line (scan-template-v4.py:299-300, :312-314) and left out.  ``names``,
    ``face_labels`` and ``person_id_maps`` are per slot, in the dict's order."""

    def __init__(self, models, device=0):
        self.device = device
        self.models = models
        self.refresh()

    def refresh(self):
        """(Re-)upload every model: call after editing the model dicts in place."""
        eng = get_engine(self.device)
        eng.bank_clear()
        self.names, self.face_labels, self.person_id_maps = [], [], []
        d = None
        for person_name, info in self.models.items():
            md = info["model_data"] if isinstance(info, dict) and "model_data" in info else info
            if md is None:
                continue
            try:
                mu, w = _folded(md)
                g = np.ascontiguousarray(md["face_features"], dtype=np.float32)
                labels, pmap = md["face_labels"], md["person_id_map"]
                if d is not None and mu.shape[0] != d:
                    raise ValueError(f"model has {mu.shape[0]} pixels, the bank {d}")
                eng.bank_add(mu, w, g.reshape(-1, w.shape[1]))
            except Exception as e:  # noqa: BLE001 - the reference prints and continues
                print(f"Error recognizing with model {person_name}: {e}")
                continue
            d = mu.shape[0]
            self.names.append(person_name)
            self.face_labels.append(labels)
            self.person_id_maps.append(pmap)
        eng.bank_owner = self  # the shared engine has one bank: whoever filled it last owns it
        return self

    def __len__(self):
        return len(self.names)

    def recognize_rows(self, rows, threshold=0.8):
        """``rows``: (b, d) uint8 grey face rows (``preprocess_faces``) ->
        [(person_id, name, confidence)] with recognize_face_all_models' rules."""
        rows = np.asarray(rows)
        if len(rows) == 0:
            return []
        if not self.names:
            return [(-1, "unknown", 0.0)] * len(rows)
        eng = get_engine(self.device)
        if getattr(eng, "bank_owner", None) is not self:  # another bank replaced this one's slots
            self.refresh()
        idx, sim, _ = eng.bank_recognize(rows, "cosine")
        return self.label(idx, sim, threshold)

    def label(self, idx, sim, threshold=0.8):
        """recognize_face_all_models' labelling of per-slot results ``idx[b, M]`` (gallery row,
        -1 for none) and ``sim[b, M]`` (cosine similarity): [(person_id, name, confidence)]."""
        best = best_over_models(sim, "cosine")  # the labelling rule, on the returned scores
        out = []
        for p, m in enumerate(best):
            if m < 0:
                out.append((-1, "unknown", 0.0))
                continue
            conf = float(sim[p, m])
            pid, name = -1, "unknown"
            if idx[p, m] >= 0 and conf >= threshold:  # recognize_face_with_model (:278-284)
                pid = self.face_labels[m][idx[p, m]]
                for nm, v in self.person_id_maps[m].items():
                    if v == pid:
                        name = nm
                        break
            out.append((pid, name if name != "unknown" else self.names[m], conf))
        return out

    def recognize_faces(self, face_imgs, threshold=0.8):
        """recognize_faces_all_models' return value for a batch of face crops: the crops are
        preprocessed in one launch and recognised against every model in one bank call.
        ``>= threshold`` for the label, the model's person name when the label is "unknown",
        (-1, "unknown", 0.0) when no model scores above 0."""
        if len(face_imgs) == 0:
            return []
        return self.recognize_rows(preprocess_faces(face_imgs, self.device), threshold)
