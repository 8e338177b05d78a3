"""Float64 dense reference for several target columns on one factorisation (dsmgp_solve_targets / dsmgp_predict_targets),
and the tolerances of their tests.

`reference(F, Y, mean, Ktn)` restates the three results from a lower Cholesky factor F of K_y (a context's download_factor, or
SciPy's factor of kernel_matrix + (noise + 1e-8) I), the leaf's rows of the targets Y (n x Q) and the per-column means:
    Z = F^-1 (Y - mean),   mll_j = -(|Z[:, j]|^2 + 2 sum log F_ii + n log 2pi) / 2,   mu = mean + Ktn F^-T Z.

Tolerances (nothing hand-picked: each is the error of the operation, with the constants tests/pred_tolerance.py already uses).

Z.  The computed factor is the exact factor of K_y + E with |E| <= c n eps |K_y| (backward stability of Cholesky); by the
perturbation bound of the Cholesky factor (Sun 1991, Stewart 1993) its relative distance to the factor of K_y itself is at
most cond_2(K_y) |E| / |K_y| / sqrt 2.  The substitution on it is backward stable too, with forward error cond_2(F) n eps |Z|
and cond_2(F) = sqrt cond_2(K_y) <= cond_2(K_y).  Both are of the form  c cond_2(K_y) eps |Z|:  with the constant 64 of
pred_tolerance.alpha_tol / mll_tol (alpha = F^-T Z is one more substitution of the same kind),
    z_tol[j] = max(1e-13, 64 cond_2(K_y) eps max_i |Z[i, j]|)                 per column.
cond_2(K_y) is taken from the factor: cond_2(F)^2 (`factor_cond`).

mll.  d(|z|^2 / 2) = z . dz, bounded entry by entry by sum_i |z_i| z_tol -- |Z|^2 carried through -- and the log-determinant
term by pred_tolerance.mll_tol's rule on its own magnitude, 64 cond_2(K_y) eps max(1, |sum log F_ii|):
    mll_tol[j] = sum_i |Z[i, j]| z_tol[j] + max(1e-13, 64 cond eps max(1, |sum_i log F_ii|)).

mu.  pred_tolerance.moment_tol: RTOL |mu| + ATOL max(1, max |Y[:, j]|), the scale of the column.

Where BOTH sides are float64 (the device against this module) each side rounds: the tests double the tolerance there, as
tests/test_loo_gpu.py does; against the 50-digit fixture it is used as it is."""
import os

import numpy as np
import scipy.linalg as sla

from pred_tolerance import ATOL, EPS, LOG2PI, RTOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    z = np.load(os.path.join(GOLDEN, "gp_targets.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = z[key]
    for c in cases.values():
        c["kind"], c["logNoise"], c["cond"] = int(c["meta"][0]), float(c["meta"][1]), float(c["meta"][2])
    return cases


def factor_cond(F):
    """cond_2(K_y) from its lower factor: cond_2(F)^2."""
    s = np.linalg.svd(np.tril(np.asarray(F, dtype=np.float64)), compute_uv=False)
    return float((s[0] / s[-1]) ** 2)


def reference(F, Y, mean, Ktn=None):
    """(Z, mll, mu) in float64; mu is None without Ktn (n_t x n)."""
    F = np.tril(np.asarray(F, dtype=np.float64))
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (Y.shape[1],))
    n = F.shape[0]
    Z = sla.solve_triangular(F, Y - mean[None, :], lower=True)
    logdet = 2.0 * np.sum(np.log(np.diag(F)))
    mll = -(np.sum(Z * Z, axis=0) + logdet + LOG2PI * n) / 2.0
    mu = None
    if Ktn is not None:
        A = sla.solve_triangular(F, Z, lower=True, trans="T")
        mu = mean[None, :] + np.asarray(Ktn, dtype=np.float64) @ A
    return Z, mll, mu


def z_tol(Z, cond):
    """Per column, broadcast over the rows (module docstring)."""
    Z = np.asarray(Z, dtype=np.float64)
    return np.broadcast_to(np.maximum(1e-13, 64.0 * cond * EPS * np.max(np.abs(Z), axis=0))[None, :], Z.shape)


def mll_tol(Z, F, cond):
    Z = np.asarray(Z, dtype=np.float64)
    hl = abs(float(np.sum(np.log(np.diag(F)))))
    return np.sum(np.abs(Z), axis=0) * z_tol(Z, cond)[0] + max(1e-13, 64.0 * cond * EPS * max(1.0, hl))


def mu_tol(mu, Y):
    """pred_tolerance.moment_tol's mean half, column by column."""
    mu = np.asarray(mu, dtype=np.float64)
    yscale = np.maximum(1.0, np.max(np.abs(np.asarray(Y, dtype=np.float64)), axis=0))
    return RTOL * np.abs(mu) + ATOL * yscale[None, :]
