"""Float64 dense restatement of k-fold cross-validation of one exact GP from a single fit (the multiple-fold residual formulas,
e.g. Ginsbourger & Schaerer 2021) and the tolerances of the k-fold tests, in one place.

With K_y = K + (noise + 1e-8) I = L L' the matrix the fit factorises, G = K_y^-1, alpha = G (y - m) and F the positions with one
label, the mean m and the hyper-parameters held fixed, the GP fitted without the rows of F predicts them jointly as

    mu_F   = y_F - G_FF^-1 alpha_F
    Sigma_F = G_FF^-1
    lpd_F  = log N(y_F | mu_F, Sigma_F) = -1/2 alpha_F' G_FF^-1 alpha_F + 1/2 log det G_FF - (|F| / 2) log 2 pi

`kfold_from_factor` evaluates exactly that from a Cholesky factor (dense_gp.factor, or a device's); `kfold_brute` is the
definition: refit without the fold (same mean, same hyper-parameters, same jitter) and predict its rows jointly -- Sigma_F
carries the noise and the 1e-8 jitter on its diagonal, as the Schur complement of K_y does.  Rows with label -1 belong to no
block: NaN moments.  An empty block has lpd 0.

Tolerances.  mu and var are predictive moments: pred_tolerance.moment_tol as it stands (`moment_tols`), doubled by the caller
where the reference is formed from a downloaded device factor (both sides round: test_loo_gpu's convention).
The joint lpd has no bound derived entry by entry.  Against the 50-digit fixture (`lpd_tol_fixture`): 16 x the error the
fixture's generator recorded for this float64 helper on the same case (tests/golden/make_kfold_golden.py), floored at
(8 + m / 256) eps sum|terms|, the rounding of a sum of m terms of that size; 16 because the device solves panels through explicit
inverses of diagonal blocks (about ten times a substitution's error, the comment in chol_blocks_plan) and sums by tiles in
another order.  Against this helper on a downloaded factor, where no error is recorded (`lpd_tol_backward`): both sides are
backward stable in K_y, i.e. exact for K_y + E with |E|_2 <= n eps |K_y|_2; lpd_F = mll(all rows) - mll(rows outside F), and
d mll = 1/2 (alpha alpha' - K_y^-1) : E, so |d lpd_F| <= n eps |K_y|_2 (|alpha|^2 + tr K_y^-1) <= n eps (|alpha|^2 |K_y|_2 +
n cond_2(K_y)), the two log marginals contributing a half each; the caller doubles it (both sides round)."""
import numpy as np
import scipy.linalg as sla

import dense_gp
import dense_kernels as dk
from dense_kernels import JITTER  # noqa: F401
from pred_tolerance import EPS, LOG2PI, moment_tol


def load_cases():
    """The cases of tests/golden/gp_kfold.npz by name: X, y, loghyp, labels (int32, n), the 50-digit mu / var (n, NaN where the
    label is -1) and lpd (K), kss, lpd_abs (K: sum of the absolute terms of every block's density), lpd_err (K: the error of the
    float64 dense helper against 50 digits, per block), and the scalars of `meta` (kind, mean, logNoise, cond_2(K_y), K, and
    `lpd_err_case`: the helper's error on the case, the largest of its blocks')."""
    cases = dk.load_cases("gp_kfold.npz")
    for c in cases.values():
        m = c.pop("meta")
        c.update(kind=int(m[0]), mean=float(m[1]), logNoise=float(m[2]), cond=float(m[3]), K=int(m[4]), lpd_err_case=float(m[5]))
        c["labels"] = np.asarray(c["labels"], dtype=np.int32)
    return cases


def blocks(labels, K):
    """The positions of every label 0 .. K - 1, ascending."""
    labels = np.asarray(labels)
    return [np.flatnonzero(labels == k) for k in range(int(K))]


def kfold_from_G(G, alpha, y, labels, K):
    """(mu, var, lpd[K], lpd_abs[K]) from G = K_y^-1 and alpha; lpd_abs = the sum of the absolute values of the terms of lpd."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    mu, var = np.full(n, np.nan), np.full(n, np.nan)
    lpd, lab = np.zeros(int(K)), np.zeros(int(K))
    for k, F in enumerate(blocks(labels, K)):
        if F.size == 0:
            continue
        C = sla.cholesky(G[np.ix_(F, F)], lower=True)
        w = sla.solve_triangular(C, alpha[F], lower=True)
        mu[F] = y[F] - sla.solve_triangular(C, w, lower=True, trans="T")
        Cinv = sla.solve_triangular(C, np.eye(F.size), lower=True)
        var[F] = np.sum(Cinv * Cinv, axis=0)
        logc = np.log(np.diag(C))
        lpd[k] = -0.5 * float(w @ w) + float(np.sum(logc)) - 0.5 * F.size * LOG2PI
        lab[k] = 0.5 * float(w @ w) + float(np.sum(np.abs(logc))) + 0.5 * F.size * LOG2PI
    return mu, var, lpd, lab


def kfold_from_factor(Lf, y, mean, labels, K):
    """(mu, var, lpd[K]) from the lower Cholesky factor of K_y."""
    Lf = np.tril(np.asarray(Lf, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64)
    Linv = sla.solve_triangular(Lf, np.eye(y.size), lower=True)
    G = Linv.T @ Linv
    alpha = sla.solve_triangular(Lf, sla.solve_triangular(Lf, y - mean, lower=True), lower=True, trans="T")
    return kfold_from_G(G, alpha, y, labels, K)[:3]


def kfold_dense(Kmat, noise, y, mean, labels, K):
    """The same from the kernel matrix (without noise) and noise = exp(2 logNoise)."""
    return kfold_from_factor(dense_gp.factor(Kmat, noise), y, mean, labels, K)


def kfold_brute(Kmat, noise, y, mean, labels, K):
    """The definition: for every label the GP fitted on the other rows (K_y without the fold's rows and columns, jitter included)
    predicts the fold's rows jointly: mu = m + K_Fr K_y,rr^-1 (y_r - m), Sigma = K_y,FF - K_Fr K_y,rr^-1 K_rF, lpd = log N(y_F |
    mu, Sigma).  A fold that holds every row is predicted by the prior: mu = m, Sigma = K_y,FF."""
    Kmat = np.asarray(Kmat, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    Ky = dk.noisy(Kmat, noise)
    mu, var, lpd = np.full(n, np.nan), np.full(n, np.nan), np.zeros(int(K))
    for k, F in enumerate(blocks(labels, K)):
        if F.size == 0:
            continue
        rest = np.setdiff1d(np.arange(n), F)
        m, S = np.full(F.size, float(mean)), Ky[np.ix_(F, F)].copy()
        if rest.size:
            cf = (dense_gp.factor(Kmat[np.ix_(rest, rest)], noise), True)
            Kfr = Kmat[np.ix_(F, rest)]
            m = m + Kfr @ sla.cho_solve(cf, y[rest] - mean)
            S = S - Kfr @ sla.cho_solve(cf, Kfr.T)
        mu[F], var[F] = m, np.diag(S)
        C = sla.cholesky(S, lower=True)
        r = sla.solve_triangular(C, y[F] - m, lower=True)
        lpd[k] = -0.5 * float(r @ r) - float(np.sum(np.log(np.diag(C)))) - 0.5 * F.size * LOG2PI
    return mu, var, lpd


def moment_tols(y, mu, var, kss, noise):
    """(tol mu, tol var) at reference moments of one leaf: pred_tolerance.moment_tol (NaN where the reference is NaN)."""
    y = np.asarray(y, dtype=np.float64)
    yscale = max(1.0, float(np.max(np.abs(y)))) if y.size else 1.0
    return moment_tol(mu, var, kss, noise, yscale)


def lpd_floor(m, lpd_abs):
    return (8.0 + np.asarray(m, dtype=np.float64) / 256.0) * EPS * np.asarray(lpd_abs, dtype=np.float64)


def lpd_tol_fixture(m, lpd_abs, lpd_err):
    """Per block, against the 50-digit value: 16 x the dense helper's recorded error on the case (`lpd_err_case` of the fixture's
    meta), floored at (8 + m / 256) eps sum|terms|."""
    return np.maximum(16.0 * np.asarray(lpd_err, dtype=np.float64), lpd_floor(m, lpd_abs))


def lpd_tol_backward(n, cond, alpha, normK):
    """Per block, against this helper on the same factor: n eps (|alpha|^2 |K_y|_2 + n cond_2(K_y)) (the module docstring)."""
    return n * EPS * (float(np.dot(alpha, alpha)) * normK + n * cond)


def factor_stats(Lf):
    """(cond_2(K_y), |K_y|_2) of K_y = Lf Lf'."""
    s = np.linalg.svd(np.tril(np.asarray(Lf, dtype=np.float64)), compute_uv=False)
    return float((s[0] / s[-1]) ** 2), float(s[0] ** 2)


def check_leaf(got_mu, got_var, got_lpd, Lf, y, mean, labels, K, kss, noise, factor=2.0):
    """One leaf of a device result against the helper on its downloaded factor `Lf`: the worst err / tol of (mu, var, lpd) with
    the moments' tolerance and lpd_tol_backward, each times `factor`; NaN patterns must agree."""
    y = np.asarray(y, dtype=np.float64)
    Lf = np.tril(np.asarray(Lf, dtype=np.float64))
    rm, rv, rl = kfold_from_factor(Lf, y, mean, labels, K)
    held = np.asarray(labels) >= 0
    assert np.array_equal(np.isnan(got_mu), ~held) and np.array_equal(np.isnan(got_var), ~held)
    tm, tv = moment_tols(y, rm, rv, kss, noise)
    cond, normK = factor_stats(Lf)
    alpha = sla.solve_triangular(Lf, sla.solve_triangular(Lf, y - mean, lower=True), lower=True, trans="T")
    tl = lpd_tol_backward(y.size, cond, alpha, normK)
    r = [0.0, 0.0, 0.0]
    if held.any():
        r[0] = float(np.max(np.abs(got_mu[held] - rm[held]) / (factor * tm[held])))
        r[1] = float(np.max(np.abs(got_var[held] - rv[held]) / (factor * tv[held])))
    r[2] = float(np.max(np.abs(np.asarray(got_lpd) - rl) / (factor * tl)))
    return r
