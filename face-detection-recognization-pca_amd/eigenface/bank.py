"""Model bank: every per-person model of the scanner resident on the GPU at once.

``MultiModelFaceScanner.recognize_face_all_models`` (scan-template-v4.py:289-319) loops over
the per-person models for every face: each has its own scaler + PCA and its own small gallery,
and the best cosine similarity is kept under a strict ``>``.  :class:`ModelBank` uploads all of
them once (``Engine.bank_add``) and answers a batch of faces with one ``ef_bank_recognize``
call, whose launch count does not depend on the number of models.

With ``face_gate`` the bank also asks Turk-Pentland's question "is this crop a face at all?" of
every model in the same call (``ef_bank_recognize_gated``): a model whose face space the crop
lies too far from takes no part in the choice over models.
"""
from __future__ import annotations

import numpy as np

from .compat import _folded, preprocess_faces
from .pca import get_engine


def best_over_models(scores, metric="cosine", allowed=None):
    """The reference's choice over models (scan-template-v4.py:293-309) for a table
    ``scores[b, M]`` of per-model best scores: walk the models in order, a model wins only
    with a strictly greater value than the best so far.  Cosine: the value is the similarity
    and the walk starts from 0.0, so nothing wins without a similarity > 0.  L2: the value is
    the negated distance and the walk starts from -inf, so the first smallest distance wins.
    NaN (an empty gallery) never wins.  ``allowed`` (b, M) bool, optional: a slot that is not
    allowed is skipped (the face gate, :func:`face_gate_mask`).  Returns int32 slots, -1 where
    no model wins."""
    s = np.asarray(scores, dtype=np.float32)
    if s.ndim != 2:
        raise ValueError("scores must be (b, M)")
    ok = None if allowed is None else np.asarray(allowed, dtype=bool)
    if ok is not None and ok.shape != s.shape:
        raise ValueError(f"allowed must be {s.shape}, got {ok.shape}")
    l2 = str(metric).lower() == "l2"
    out = np.full(s.shape[0], -1, np.int32)
    for p in range(s.shape[0]):
        best = np.float32(-np.inf) if l2 else np.float32(0.0)
        for m in range(s.shape[1]):
            if ok is not None and not ok[p, m]:
                continue
            v = -s[p, m] if l2 else s[p, m]
            if v > best:  # False for NaN
                best = v
                out[p] = m
    return out


def face_gate_mask(dffs2, energy, gate, relative=True):
    """The face gate's decision, exactly as ``ef_bank_recognize_gated`` makes it: slot m is
    rejected for probe p when ``dffs2[p, m] > bound`` is true, with ``bound = gate[m]`` or, when
    ``relative``, the float32 product ``gate[m] * energy[p, m]``.  The comparison is false for
    NaN, so a gate of +inf or NaN rejects nothing.  Returns allowed (b, M) bool."""
    e2 = np.asarray(dffs2, dtype=np.float32)
    g = np.broadcast_to(np.asarray(gate, dtype=np.float32), e2.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        bound = g * np.asarray(energy, dtype=np.float32) if relative else g
        return ~(e2 > bound)


def _operands(md):
    """(mean, W, components (k, d), scaler scale or None) of a model dict: the ``face_model.pkl``
    layout (``pca`` + ``scaler``, folded), or the ``models/*_pca_model.pkl`` layout
    (``eigenfaces`` (d, k) + ``mean_face``).  A dict with neither raises KeyError('pca')."""
    if "pca" not in md and "eigenfaces" in md:
        w = np.ascontiguousarray(md["eigenfaces"], dtype=np.float32)
        return np.ascontiguousarray(md["mean_face"], dtype=np.float32), w, w.T, None
    mu, w = _folded(md)
    return mu, w, md["pca"].components_, md["scaler"].scale_


class ModelBank:
    """The scanner's models (the dict ``load_all_models`` returns, or ``{name: model_data}``)
    as one resident bank.  A model that is ``None`` is left out silently and one that fails
    to fold or upload is reported with the reference's ``Error recognizing with model
    {name}: {e}`` line (scan-template-v4.py:299-300, :312-314) and left out.  ``names``,
    ``face_labels`` and ``person_id_maps`` are per slot, in the dict's order.

    ``face_gate``: a float, one relative bound eps^2 / E on the distance from face space for
    every model, or a ``{name: bound}`` dict (a missing name: no gate for that model).  A face
    that a model's gate rejects is never labelled by that model; one that no model accepts is
    ``(-1, "unknown", 0.0)``.  None: no gate, and nothing of it is uploaded."""

    def __init__(self, models, device=0, face_gate=None):
        self.device = device
        self.models = models
        self.face_gate = face_gate
        self.refresh()

    def refresh(self):
        """(Re-)upload every model: call after editing the model dicts in place."""
        eng = get_engine(self.device)
        eng.bank_clear()
        self.names, self.face_labels, self.person_id_maps = [], [], []
        self._recon_src, self._recon_up = [], False
        d = None
        for person_name, info in self.models.items():
            md = info["model_data"] if isinstance(info, dict) and "model_data" in info else info
            if md is None:
                continue
            try:
                mu, w, comps, scale = _operands(md)
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
            self._recon_src.append((comps, scale))
        if self.face_gate is None:
            self.gate, self.gated = None, np.zeros(len(self.names), bool)
        elif isinstance(self.face_gate, dict):
            self.gated = np.array([n in self.face_gate for n in self.names], bool)
            self.gate = np.array([self.face_gate.get(n, np.inf) for n in self.names], np.float32)
        else:
            self.gated = np.ones(len(self.names), bool)
            self.gate = np.full(len(self.names), self.face_gate, np.float32)
        if self.face_gate is not None:
            self._upload_reconstruction(eng)
        eng.bank_owner = self  # the shared engine has one bank: whoever filled it last owns it
        return self

    def _upload_reconstruction(self, eng):
        """Every slot's way back (R, s), from the operands its projection was folded from."""
        from .pca import reconstruction_operands
        for slot, (comps, scale) in enumerate(self._recon_src):
            eng.bank_set_reconstruction(slot, *reconstruction_operands(comps, scale))
        self._recon_up = True

    def _engine(self, reconstruction=False):
        eng = get_engine(self.device)
        if getattr(eng, "bank_owner", None) is not self:  # another bank replaced this one's slots
            self.refresh()
        if reconstruction and not self._recon_up:
            self._upload_reconstruction(eng)
        return eng

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
        if self.gate is None:
            idx, sim, _ = self._engine().bank_recognize(rows, "cosine")
            return self.label(idx, sim, threshold)
        idx, sim, _, eps2, energy = self._engine(True).bank_recognize_gated(rows, self.gate, "cosine", relative=True)
        return self.label(idx, sim, threshold, allowed=face_gate_mask(eps2, energy, self.gate))

    def face_distance(self, rows):
        """(eps2, energy), float64 (b, M): per model the squared distance from its face space of
        every row and the row's energy about the model's mean, as ``compat.face_space_distance``
        measures them per model (``face_model.pkl`` dicts in the scaler's space).  Uploads the
        models' ways back on first use, gate or no gate."""
        rows = np.asarray(rows)
        if len(rows) == 0 or not self.names:
            return np.zeros((len(rows), len(self.names))), np.zeros((len(rows), len(self.names)))
        eng = self._engine(True)
        chunk = 4096  # EF_BANK_MAX_PROBES
        parts = [eng.bank_face_distance(rows[o:o + chunk], return_energy=True) for o in range(0, len(rows), chunk)]
        return (np.concatenate([p[0] for p in parts]).astype(np.float64),
                np.concatenate([p[1] for p in parts]).astype(np.float64))

    def is_face(self, rows):
        """bool (b,): True where at least one gated model accepts the row as a face."""
        if self.gate is None:
            raise ValueError("is_face needs a face_gate")
        rows = np.asarray(rows)
        if len(rows) == 0 or not self.names:
            return np.zeros(len(rows), bool)
        eng = self._engine(True)
        chunk = 4096
        out = []
        for o in range(0, len(rows), chunk):
            eps2, energy = eng.bank_face_distance(rows[o:o + chunk], return_energy=True)
            out.append((face_gate_mask(eps2, energy, self.gate) & self.gated[None, :]).any(axis=1))
        return np.concatenate(out)

    def label(self, idx, sim, threshold=0.8, allowed=None):
        """recognize_face_all_models' labelling of per-slot results ``idx[b, M]`` (gallery row,
        -1 for none) and ``sim[b, M]`` (cosine similarity): [(person_id, name, confidence)].
        ``allowed`` (b, M) bool: the face gate's mask; a slot that is not allowed never wins."""
        best = best_over_models(sim, "cosine", allowed)  # the labelling rule, on the returned scores
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
