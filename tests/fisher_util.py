"""Host references for the Fisher discriminant tests: the case generator, the class
statistics from their definition in np.longdouble, the generalised eigenproblem through
scipy.linalg.eigh, and the four accuracy figures the fit is held to."""
import functools

import numpy as np

EPS = 2.0 ** -52
CLUSTER = 1e-6  # eigenvalues closer than this (relative to the largest) form one cluster


def lighting_case(k=32, n_classes=10, per=30, seed=0):
    """Identity centres 0.5 N(0, I), within-person noise 0.4 N(0, I) and "lighting"
    8 N(0, I_3) along three random orthonormal directions shared by everybody; the rows are
    shuffled, so the labels arrive interleaved.  (features (n, k) float64, labels (n,) int32)"""
    rng = np.random.default_rng(seed)
    centres = 0.5 * rng.standard_normal((n_classes, k))
    u, _ = np.linalg.qr(rng.standard_normal((k, min(3, k))))
    labels = np.repeat(np.arange(n_classes), per)
    n = labels.size
    f = centres[labels] + 0.4 * rng.standard_normal((n, k)) + (8.0 * rng.standard_normal((n, u.shape[1]))) @ u.T
    p = rng.permutation(n)
    return np.ascontiguousarray(f[p]), labels[p].astype(np.int32)


def ref_scatter(F, labels, n_classes):
    """counts, mean, class_means (zero rows for empty classes), Sw, Sb from the definition in
    np.longdouble, and the magnitudes the error bounds are stated in: abs_class[c][j] =
    sum_{i in c} |f_ij|, abs_prod[a][b] = sum_i |f_ia - m_a| |f_ib - m_b|."""
    f = np.asarray(F).astype(np.longdouble)
    n, k = f.shape
    m = f.sum(axis=0) / n
    counts = np.bincount(labels, minlength=n_classes).astype(np.int64)
    M = np.zeros((n_classes, k), np.longdouble)
    abs_class = np.zeros((n_classes, k))
    for c in np.flatnonzero(counts):
        rows = f[labels == c]
        M[c] = rows.sum(axis=0) / counts[c]
        abs_class[c] = np.abs(rows).sum(axis=0).astype(np.float64)
    xc = f - M[labels]
    Sw = xc.T @ xc
    d = (M - m) * (counts > 0)[:, None]
    Sb = d.T @ (d * counts[:, None].astype(np.longdouble))
    a = np.abs((f - m).astype(np.float64))
    return {"counts": counts, "mean": m, "class_means": M, "Sw": Sw, "Sb": Sb, "abs_class": abs_class,
            "abs_prod": a.T @ a}


def shrink(Sw, gamma):
    k = Sw.shape[0]
    return (1.0 - gamma) * Sw + gamma * np.trace(Sw) / k * np.eye(k)


def sign_fix(A):
    """In each column the entry of largest magnitude positive, first index on ties."""
    i = np.argmax(np.abs(A), axis=0)
    s = np.where(A[i, np.arange(A.shape[1])] < 0, -1.0, 1.0)
    return A * s[None, :]


def ref_fit(Sw_g, Sb, dof):
    """All k eigenpairs of (Sb, Sw_g) by scipy.linalg.eigh in fp64: eigenvalues descending,
    A^T (Sw_g / dof) A = I, the sign rule."""
    import scipy.linalg
    w, v = scipy.linalg.eigh(np.asarray(Sb, np.float64), np.asarray(Sw_g, np.float64))
    o = np.argsort(-w, kind="stable")
    return sign_fix(v[:, o] * np.sqrt(dof)), w[o]


def alt_fit(Sw_g, Sb, dof):
    """The same eigenpairs by another order of operations (Cholesky, two triangular solves,
    the standard symmetric solver): what scipy's own solution is compared with."""
    import scipy.linalg
    L = np.linalg.cholesky(np.asarray(Sw_g, np.float64))
    X = scipy.linalg.solve_triangular(L, np.asarray(Sb, np.float64), lower=True)
    T = scipy.linalg.solve_triangular(L, X.T, lower=True)
    w, v = np.linalg.eigh(0.5 * (T + T.T))
    o = np.argsort(-w, kind="stable")
    A = scipy.linalg.solve_triangular(L.T, v[:, o], lower=False)
    return sign_fix(A * np.sqrt(dof)), w[o]


def span_residual(A, ref_A, ref_lam, m):
    """Largest residual of a column of A[:, :m] regressed on the reference columns of its own
    cluster of near-equal eigenvalues, relative to the column's norm and weighted with the
    cluster's distance to the rest of the spectrum over lambda_1 (an invariant subspace moves by
    (perturbation) / (gap), Davis-Kahan; the weight takes the gap out again)."""
    lam1 = ref_lam[0]
    k = ref_lam.size
    worst, i = 0.0, 0
    while i < m:
        j = i + 1
        while j < k and ref_lam[j - 1] - ref_lam[j] <= CLUSTER * lam1:
            j += 1
        gap = min(ref_lam[i - 1] - ref_lam[i] if i > 0 else np.inf, ref_lam[j - 1] - ref_lam[j] if j < k else np.inf)
        R, cols = ref_A[:, i:j], A[:, i:min(j, m)]
        coef = np.linalg.lstsq(R, cols, rcond=None)[0]
        res = np.linalg.norm(cols - R @ coef, axis=0) / np.linalg.norm(cols, axis=0)
        worst = max(worst, float(res.max()) * min(gap / lam1, 1.0))
        i = j
    return worst


def fit_figures(A, lam, Sw_g, Sb, dof, ref_A, ref_lam):
    """The four figures of a solution A (k, m), lam (m,) against the host's long-double
    scatters: the normalisation, the diagonalisation, the eigenvalues, the span."""
    m = A.shape[1]
    Al = A.astype(np.longdouble)
    lam1 = float(ref_lam[0])
    q1 = float(np.abs(Al.T @ (Sw_g / dof) @ Al - np.eye(m)).max())
    q2 = float(np.abs(Al.T @ Sb @ Al / dof - np.diag(lam.astype(np.longdouble))).max()) / lam1
    q3 = float(np.abs(lam - ref_lam[:m]).max()) / lam1
    q4 = span_residual(A, ref_A, ref_lam, m)
    return np.array([q1, q2, q3, q4])


# ---- the fit cases: name -> (k, classes, rows per class, shrinkage, seed) ----------------
FIT_CASES = {
    "lighting": (32, 10, 30, 0.0, 0),
    "k128": (128, 10, 30, 0.0, 0),
    "tiny": (8, 3, 5, 0.0, 0),
    "two_classes": (16, 2, 30, 0.0, 0),
    "k256": (256, 10, 60, 0.0, 0),
    "shrunk": (100, 10, 8, 0.1, 0),  # n - C = 70 < k: singular without shrinkage
}


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """Everything host-side of one fit case, computed once."""
    k, C, per, gamma, seed = FIT_CASES[name]
    F, labels = lighting_case(k, C, per, seed)
    sc = ref_scatter(F, labels, C)
    dof = F.shape[0] - C
    Sw_g = shrink(sc["Sw"], gamma)
    cond = float(np.linalg.cond(Sw_g.astype(np.float64)))
    ref_A, ref_lam = ref_fit(Sw_g, sc["Sb"], dof)
    alt_A, alt_lam = alt_fit(Sw_g, sc["Sb"], dof)
    m = min(k, C - 1)
    unit = k * EPS * cond
    # scipy's own solution: normalisation and diagonalisation against the long-double
    # scatters, eigenvalues and span against the other order of operations
    ref_fig = fit_figures(ref_A[:, :m], ref_lam[:m], Sw_g, sc["Sb"], dof, alt_A, alt_lam)
    return {"F": F, "labels": labels, "C": C, "gamma": gamma, "m": m, "dof": dof, "Sw_g": Sw_g, "Sb": sc["Sb"],
            "cond": cond, "ref_A": ref_A, "ref_lam": ref_lam, "unit": unit, "ref_fig": ref_fig}


@functools.lru_cache(maxsize=None)
def fit_constant():
    """c of the bound c k 2^-52 cond(Sw_g): the smallest with which scipy's own solution
    passes every figure of every case with 4x headroom."""
    return 4.0 * max(float((fit_case(n)["ref_fig"] / fit_case(n)["unit"]).max()) for n in FIT_CASES)


def pca_host(X, k):
    """(mean, W (d, k), features (n, k)) of the eigenface step on the host (SVD, fp64)."""
    x = np.asarray(X, np.float64)
    mu = x.mean(axis=0)
    _, _, vt = np.linalg.svd(x - mu, full_matrices=False)
    W = vt[:k].T
    return mu, W, (x - mu) @ W


def render_pixels(F, side=24, scale=4.0, seed=0):
    """uint8 faces whose pixels carry the features: mean_face + scale F B^T for an orthonormal
    basis B of the image; rounding to uint8 adds 0.29 / scale per feature, well under the 0.4
    noise of the lighting case."""
    from eigenface import synth
    B = synth.basis(side * side, F.shape[1], seed)
    x = synth.mean_face(side)[None, :] + scale * (F @ B.T)
    assert x.min() >= 0.0 and x.max() <= 255.0
    return np.rint(x).astype(np.uint8)
