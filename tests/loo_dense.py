"""Float64 dense restatement of leave-one-out cross-validation of one exact GP (Rasmussen & Williams, GPML 5.4.2, eqs. 5.10-5.12)
and the tolerances of the LOO tests, in one place.

With K_y = K + (noise + 1e-8) I = L L' the matrix the fit factorises, d_i = [K_y^-1]_ii = |column i of L^-1|^2 and
alpha = K_y^-1 (y - m), the mean m and the hyper-parameters held fixed:

    mu_loo_i  = y_i - alpha_i / d_i
    var_loo_i = 1 / d_i
    lpd_i     = -(log 2pi + log var_loo_i + (y_i - mu_loo_i)^2 / var_loo_i) / 2

`loo_from_factor` evaluates exactly that from a Cholesky factor (dense_gp.factor, or a device's), `loo_brute` is the definition: refit without row i
(same mean, same hyper-parameters, same jitter) and predict at x_i.  var_loo_i is that fit's k(x_i, x_i) - |v|^2 + noise plus
the 1e-8 jitter; mu_loo_i is its mean.

Tolerances (`loo_tol`): LOO moments are predictive moments, so pred_tolerance.moment_tol applies as it stands --
RTOL |mu| + ATOL max(1, max|y|) and RTOL |var| + ATOL max(1, k(x_i, x_i) + noise); lpd_i gets both carried through its formula
(pred_tolerance.Prop), the leaf sum their sum plus (8 + n / 256) eps times the mean |lpd_i| for the rounding of the sum itself."""
import numpy as np
import scipy.linalg as sla

import dense_gp
import dense_kernels as dk
from dense_kernels import JITTER  # noqa: F401  (the tests read it from here)
from pred_tolerance import EPS, LOG2PI, Prop, moment_tol


def load_cases():
    """The cases of tests/golden/gp_loo.npz by name: X, y, loghyp, the 50-digit mu / var / lpd (per row) and kss, and the
    scalars of `meta` (kind, mean, logNoise, cond_2(K_y), the 50-digit sum of lpd)."""
    cases = dk.load_cases("gp_loo.npz")
    for c in cases.values():
        m = c.pop("meta")
        c.update(kind=int(m[0]), mean=float(m[1]), logNoise=float(m[2]), cond=float(m[3]), lpd_sum=float(m[4]))
    return cases


def lpd_terms(y, mu, var):
    """lpd_i over any arithmetic with log as a method or through numpy (float64 arrays or Prop)."""
    d = y - mu
    lv = var.log() if isinstance(var, Prop) else np.log(var)
    return (lv + d * d / var + LOG2PI) * -0.5


def loo_from_factor(Lf, y, mean):
    """(mu_loo, var_loo, lpd_i) from the lower Cholesky factor of K_y."""
    Lf = np.tril(np.asarray(Lf, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    Linv = sla.solve_triangular(Lf, np.eye(n), lower=True)
    d = np.sum(Linv * Linv, axis=0)
    alpha = sla.solve_triangular(Lf, sla.solve_triangular(Lf, y - mean, lower=True), lower=True, trans="T")
    mu = y - alpha / d
    var = 1.0 / d
    return mu, var, lpd_terms(y, mu, var)


def loo_dense(K, noise, y, mean):
    """The same from the kernel matrix K (without noise) and noise = exp(2 logNoise)."""
    return loo_from_factor(dense_gp.factor(K, noise), y, mean)


def loo_brute(K, noise, y, mean):
    """The definition: for every i the GP fitted on the other rows (K_y without row and column i, jitter included) predicts
    x_i: mu = m + k_i' K_y,-i^-1 (y_-i - m), var = K_ii - k_i' K_y,-i^-1 k_i + noise (no jitter: a predictive variance)."""
    K = np.asarray(K, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    mu = np.empty(n)
    var = np.empty(n)
    for i in range(n):
        keep = np.arange(n) != i
        if n == 1:
            mu[i], var[i] = mean, K[i, i] + noise
            continue
        cf = (dense_gp.factor(K[np.ix_(keep, keep)], noise), True)
        ki = K[keep, i]
        mu[i] = mean + ki @ sla.cho_solve(cf, y[keep] - mean)
        var[i] = K[i, i] - ki @ sla.cho_solve(cf, ki) + noise
    return mu, var


def loo_tol(y, mu, var, kss, noise):
    """(tol mu, tol var, tol lpd_i, tol of the leaf sum) at reference moments (mu, var) of one leaf."""
    y = np.asarray(y, dtype=np.float64)
    yscale = max(1.0, float(np.max(np.abs(y)))) if y.size else 1.0
    tm, tv = moment_tol(mu, var, kss, noise, yscale)
    terms = lpd_terms(Prop(y), Prop(mu, tm), Prop(var, tv))
    n = y.size
    tsum = float(np.sum(terms.e)) + (8 + n / 256.0) * EPS * float(np.mean(np.abs(terms.v)))
    return tm, tv, terms.e, tsum
