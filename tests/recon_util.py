"""fp64 reference and error bounds of the back-projection (NumPy only).

    x^   = mean + f . R
    eps2 = sum_j (s_j (p_j - x^_j))^2
    E    = sum_j (s_j (p_j - mean_j))^2

Every bound is built from the projection test's constants for an fp32 MFMA product,
|error| <= 2e-6 * sum|a||b| + 1e-6, and the unit roundoff of fp32.

Residual.  The kernel forms s_j ((p_j - mean_j) - acc_j): the product acc_j carries the MFMA
error on (|F| |R|)_j, the subtractions and the multiplication one fp32 rounding each on terms no
larger than |p_j - mean_j| + (|F| |R|)_j, all far inside the 2e-6.  So per pixel

    e_j = s_j (2e-6 (|p_j - mean_j| + (|F| |R|)_j) + 1e-6)

bounds the error of the weighted residual r_j, and with r_j the fp64 residual at the same features

    |eps2 - eps2_ref| <= sum_j (2 |r_j| e_j + e_j^2) + (d + k) 2^-24 eps2_ref,

the last term being the worst-case fp32 summation of d non-negative terms in any order.  E uses
the same form with r_j = s_j (p_j - mean_j).

Reconstruction.  The kernel stores fl(mean_j + acc_j): no pixel takes part, and the operand
added to the product is mean_j, so mean_j takes the place of p_j - mean_j:

    |x^_j - x^_ref_j| <= 2e-6 (|mean_j| + (|F| |R|)_j) + 1e-6.

(The term cannot be left out: an fp32 x^ near 128 is only known to 2^-24 * 128 = 7.6e-6, more
than the 1e-6 floor, wherever (|F| |R|)_j is small.)
"""
import numpy as np

U32 = 2.0 ** -24


def f64(a):
    return np.asarray(a, dtype=np.float64)


def reconstruct_ref(F, R, mean):
    """x^ (b, d) in fp64 from the operands as stored (fp32 values)."""
    return f64(mean)[None, :] + f64(F) @ f64(R)


def residual_ref(P, F, R, mean, s=None):
    """The weighted residual r (b, d) in fp64 at the features F."""
    r = f64(P) - reconstruct_ref(F, R, mean)
    return r if s is None else r * f64(s)[None, :]


def centred_ref(P, mean, s=None):
    c = f64(P) - f64(mean)[None, :]
    return c if s is None else c * f64(s)[None, :]


def product_mag(F, R):
    return np.abs(f64(F)) @ np.abs(f64(R))


def residual_err(P, F, R, mean, s=None, extra=None):
    """e (b, d): the bound on the kernel's error in r.  extra (b, d): a further per-pixel error
    of the product, e.g. the projection's own error carried through |R|."""
    e = 2e-6 * (np.abs(f64(P) - f64(mean)[None, :]) + product_mag(F, R)) + 1e-6
    if extra is not None:
        e = e + extra
    return e if s is None else e * f64(s)[None, :]


def sumsq_bound(r, e, terms):
    """Bound on |fp32 sum of squares - sum r^2| per row, for per-element error e in r."""
    ref = (r * r).sum(axis=1)
    return (2.0 * np.abs(r) * e + e * e).sum(axis=1) + terms * U32 * ref


def recon_err(F, R, mean):
    """(b, d): the bound on |x^ - x^_ref| of the fp32 reconstruction."""
    return 2e-6 * (np.abs(f64(mean))[None, :] + product_mag(F, R)) + 1e-6


def u8_ref(xhat):
    return np.rint(np.clip(xhat, 0.0, 255.0)).astype(np.uint8)


def u8_undecided(xhat, tol):
    """Pixels whose fp64 x^ lies within tol of a half-integer inside [0, 255]: the only ones an
    fp32 result within tol may round the other way.  Clamped pixels are never among them."""
    near = np.abs(xhat - (np.floor(xhat) + 0.5)) <= tol
    inside = (xhat > 0.5 - tol) & (xhat < 254.5 + tol)
    clamped = (xhat < -0.5) | (xhat > 255.5)
    return near & inside & ~clamped


def standardised_operands(V, sigma):
    """fp64 (W (d, k), R (k, d), s (d,)) of a standardised model with orthonormal rows V (k, d)
    and scaler scale sigma (a zero counts as 1): W = diag(1/sigma) V^T, R = V diag(sigma),
    s = 1/sigma."""
    sg = f64(sigma).copy()
    sg[sg == 0.0] = 1.0
    V = f64(V)
    return (V / sg[None, :]).T.copy(), V * sg[None, :], 1.0 / sg


def orthonormal_rows(rng, k, d):
    q, _ = np.linalg.qr(rng.standard_normal((d, k)))
    return np.ascontiguousarray(q.T)
