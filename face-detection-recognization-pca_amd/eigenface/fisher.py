"""Fisherfaces (Belhumeur, Hespanha, Kriegman 1997): eigenfaces first, then a linear
discriminant inside face space that maximises between-identity over within-identity scatter.

The leading eigenfaces follow the largest variance of the training faces, and the largest
variance is usually illumination, not identity.  The discriminant re-weights face space with
the labels: its L2 distance is the within-class Mahalanobis distance.  Both steps run on the
GPU (``Engine.fit``, ``Engine.lda_fit``); the discriminant then folds into the projection
matrix, ``W' = W . A`` with the same mean, so projection, search, the model bank and the frame
scanners run a Fisher model exactly as they run an eigenface model.
"""
from __future__ import annotations

import numpy as np

from .pca import EigenfacePCA, get_engine

MAX_PCA_COMPONENTS = 256  # the discriminant's limit (ef_lda_fit)


def fold_scalings(W, A):
    """W' = W . A in float64: the projection matrix (d, k) of an eigenface model (with the
    scaler's 1/sigma already in it) times the discriminant's scalings (k, m)."""
    W = np.asarray(W, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    if W.ndim != 2 or A.ndim != 2 or W.shape[1] != A.shape[0]:
        raise ValueError(f"W must be (d, k) and A (k, m), got {W.shape} and {A.shape}")
    return W @ A


def pca_components_for(n, n_classes, pca_components=None):
    """Width of the eigenface step in front of the discriminant: min(pca_components or 256,
    n - C, 256).  n - C is Belhumeur's choice: it keeps the within-class scatter regular."""
    k = min(int(pca_components) if pca_components else MAX_PCA_COMPONENTS, n - n_classes, MAX_PCA_COMPONENTS)
    if k < 1:
        raise ValueError(f"Fisherfaces needs more rows than classes (n = {n}, classes = {n_classes})")
    return k


class Fisherfaces:
    """Fisherfaces estimator: ``EigenfacePCA`` with ``min(pca_components or 256, n - C, 256)``
    components, then the discriminant of the training projection (``n_components`` columns,
    default C - 1), folded into one projection ``(p - mean) . W'``.

    ``transform``, ``set_gallery``, ``recognize`` and ``recognize_topk`` behave as in
    ``EigenfacePCA``.  There is no ``inverse_transform``: the discriminant's scalings are not
    orthonormal (they are Sw-orthonormal), so W' has no transpose that leads back to pixels.

    After ``fit``: ``mean_`` (d,), ``scalings_`` W' (d, m) float64, ``lda_scalings_`` A (k, m),
    ``eigenvalues_`` (m,), ``classes_``, ``labels_`` (n,) as indices into ``classes_``,
    ``face_features_`` (n, m) the training rows in Fisher space, ``pca_`` the eigenface step
    and ``pca_features_`` its projection of the training rows.
    """

    def __init__(self, n_components=None, pca_components=None, standardize=False, shrinkage=0.0, device=0):
        self.n_components = n_components
        self.pca_components = pca_components
        self.standardize = standardize
        self.shrinkage = shrinkage
        self.device = device

    def fit(self, X, y):
        x = np.asarray(X)
        classes, lab = np.unique(np.asarray(y), return_inverse=True)
        lab = lab.reshape(-1)
        n = x.shape[0]
        if lab.shape[0] != n:
            raise ValueError(f"y must hold one label per row of X ({n}), got {lab.shape[0]}")
        if len(classes) < 2:
            raise ValueError("Fisherfaces needs at least two identities")
        k = pca_components_for(n, len(classes), self.pca_components)
        pca = EigenfacePCA(k, standardize=self.standardize, device=self.device).fit(x)
        r = get_engine(self.device).lda_fit(pca.face_features_, lab.astype(np.int32), self.n_components,
                                            self.shrinkage, n_classes=len(classes))
        self.pca_ = pca
        self.pca_features_ = pca.face_features_
        self.classes_, self.labels_ = classes, lab.astype(np.int32)
        self.n_samples_, self.n_features_in_ = n, x.shape[1]
        self.lda_scalings_, self.eigenvalues_ = r.scalings, r.eigenvalues
        self.n_components_ = int(r.scalings.shape[1])
        # W as EigenfacePCA folds it, kept in float64: it carries 1/sigma with the scaler
        w = (pca.components_ / pca.scaler_scale_[None, :]).T if self.standardize else pca.components_.T
        return self._set_model(pca.mean_face_, fold_scalings(w, r.scalings), pca.face_features_ @ r.scalings)

    def _set_model(self, mean, scalings, features):
        self.mean_ = np.ascontiguousarray(mean, dtype=np.float64)
        self.scalings_ = np.ascontiguousarray(scalings, dtype=np.float64)
        self.face_features_ = np.ascontiguousarray(features, dtype=np.float64)
        self._W = np.ascontiguousarray(self.scalings_, dtype=np.float32)
        self._mu = np.ascontiguousarray(self.mean_, dtype=np.float32)
        # owner tokens, as EigenfacePCA keeps them
        self._model_token = object()
        self._gallery_token = None
        self._gallery_src = None
        return self

    def fit_transform(self, X, y):
        return self.fit(X, y).face_features_

    # the resident-model and gallery logic is EigenfacePCA's, on this object's (_mu, _W)
    _ensure_model = EigenfacePCA._ensure_model
    transform = EigenfacePCA.transform
    set_gallery = EigenfacePCA.set_gallery
    save_gallery = EigenfacePCA.save_gallery
    recognize = EigenfacePCA.recognize
    recognize_topk = EigenfacePCA.recognize_topk

    # ------------------------------------------------------------------ files
    def save(self, path):
        """One ``.npz`` (no pickle): mean, W', the training features in Fisher space, their
        labels (indices into classes), the classes and the eigenvalues.  ``path`` should end in
        ``.npz`` (numpy appends it otherwise)."""
        np.savez(path, mean=self.mean_, scalings=self.scalings_, features=self.face_features_, labels=self.labels_,
                 classes=self.classes_, eigenvalues=self.eigenvalues_)
        return path

    @classmethod
    def load(cls, path, device=0):
        """The estimator ``save`` wrote, ready to ``transform`` and ``recognize`` (the eigenface
        step itself is not kept: ``pca_`` and ``lda_scalings_`` are absent)."""
        with np.load(path, allow_pickle=False) as z:
            self = cls(n_components=int(z["scalings"].shape[1]), device=device)
            self.labels_, self.classes_, self.eigenvalues_ = z["labels"], z["classes"], z["eigenvalues"]
            self.n_samples_, self.n_features_in_ = int(z["features"].shape[0]), int(z["scalings"].shape[0])
            self.n_components_ = int(z["scalings"].shape[1])
            return self._set_model(z["mean"], z["scalings"], z["features"])

    def bank_triple(self):
        """(mean (d,), W' (d, m), features (n, m)) float32: what ``Engine.bank_add`` /
        ``ModelBank`` take."""
        return self._mu, self._W, np.ascontiguousarray(self.face_features_, dtype=np.float32)
