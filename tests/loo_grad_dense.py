"""Float64 dense restatement of the hyper-parameter gradients of the leave-one-out log predictive density of one exact GP
(Rasmussen & Williams, GPML 5.4.2, eq. 5.13) and the tolerance of its tests, in one place.

With K_y = K + c I (c = exp(2 logNoise) + 1e-8, the matrix the fit factorises), G = K_y^-1, d = diag G, alpha = G (y - m) and
lpd = sum_i -(log 2pi - log d_i + alpha_i^2 / d_i) / 2 (loo_dense.loo_dense, summed), the mean m held fixed:

    literal (5.13):  dlpd/dtheta = sum_i (alpha_i [Z alpha]_i - (1 + alpha_i^2 / d_i) [Z G]_ii / 2) / d_i,   Z = G dK_y/dtheta
    M form:          dlpd/dtheta = sum_rc M_rc (dK_y/dtheta)_rc,   M = (u alpha' + alpha u') / 2 - G diag(w) G,
                     u = G (alpha / d),   w_i = (1 + alpha_i^2 / d_i) / (2 d_i)

`dKs` are the true derivatives dK/dtheta_j of dense_kernels.d_hyper; `loo_grad_dense` is the M form, `loo_grad_literal` the
literal one, both from G formed explicitly; both return the vector [dl..., (da,) ds, dnoise] of dsmgp_loo_gradients.

Tolerance (`tolerance`): the project's gradient rule as tests/test_gradients_gpu.py::_tolerance states it, per component
max(1e-13, 64 cond_2(K_y) eps max(1, |g_ref|_inf)).  dsmgp_loo_gradients contracts the signal variance and the SE / Matern
length-scales with M directly; only IsoLinear's dl = -2 (tr(M K_y) - c tr M) goes through the trace identity, whose halves
cancel when the signal is weak against c.  For a weak-signal IsoLinear case that component also gets the floor of the same
construction as there: 8 eps x the size of the cancelling halves,
sum alpha_i^2/d_i + sum w_i d_i + c (|u . alpha| + |H|_F^2), H = G diag(sqrt w)."""
import numpy as np
import scipy.linalg as sla

import dense_gp
from dense_kernels import JITTER, load_cases as _load

EPS = np.finfo(np.float64).eps


def load_cases():
    """The cases of tests/golden/gp_loo_grad.npz by name: X, y, loghyp (without the noise), grad (50 digits, [dl..., ds,
    dnoise]) and the scalars of `meta`: kind, mean, logNoise, cond_2(K_y), lpd (50 digits), weak (1: sigma^2 / c = 1e-8)."""
    cases = _load("gp_loo_grad.npz")
    for c in cases.values():
        m = c.pop("meta")
        c.update(kind=int(m[0]), mean=float(m[1]), logNoise=float(m[2]), cond=float(m[3]), lpd=float(m[4]), weak=bool(m[5]))
    return cases


def _parts(K, noise, y, mean):
    """(G, d, alpha) with G = K_y^-1 formed explicitly."""
    G = sla.cho_solve((dense_gp.factor(K, noise), True), np.eye(len(y)))
    G = 0.5 * (G + G.T)
    alpha = G @ (np.asarray(y, dtype=np.float64) - mean)
    return G, np.diag(G).copy(), alpha


def loo_grad_from_factor(F, dKs, noise, y, mean):
    """`loo_grad_dense` from a lower Cholesky factor of K_y (a downloaded device factor) in place of K."""
    F = np.tril(np.asarray(F, dtype=np.float64))
    Fi = sla.solve_triangular(F, np.eye(len(y)), lower=True)
    G = Fi.T @ Fi
    M, _ = loo_matrix(None, noise, y, mean, G=G)
    return np.array([float(np.sum(M * dK)) for dK in dKs] + [2.0 * noise * float(np.trace(M))])


def loo_matrix(K, noise, y, mean, G=None):
    """M of the M form, and (G, d, alpha, u, w); G = K_y^-1 may be given instead of K."""
    if G is None:
        G, d, alpha = _parts(K, noise, y, mean)
    else:
        d, alpha = np.diag(G).copy(), G @ (np.asarray(y, dtype=np.float64) - mean)
    u = G @ (alpha / d)
    w = (1.0 + alpha * alpha / d) / (2.0 * d)
    M = 0.5 * (np.outer(u, alpha) + np.outer(alpha, u)) - (G * w) @ G
    return M, (G, d, alpha, u, w)


def loo_grad_dense(K, dKs, noise, y, mean):
    """[sum_rc M_rc dK_j,rc ..., 2 noise tr M]: the gradient in the layout of dsmgp_loo_gradients."""
    M, _ = loo_matrix(K, noise, y, mean)
    return np.array([float(np.sum(M * dK)) for dK in dKs] + [2.0 * noise * float(np.trace(M))])


def loo_grad_literal(K, dKs, noise, y, mean):
    """GPML eq. 5.13 as printed, from G = K_y^-1 (no M)."""
    G, d, alpha = _parts(K, noise, y, mean)
    out = []
    for dK in list(dKs) + [2.0 * noise * np.eye(len(y))]:
        Z = G @ dK
        out.append(float(np.sum((alpha * (Z @ alpha) - 0.5 * (1.0 + alpha * alpha / d) * np.diag(Z @ G)) / d)))
    return np.array(out)


def lpd_sum(K, noise, y, mean):
    """sum_i lpd_i of loo_dense.loo_dense."""
    from loo_dense import loo_dense
    return float(np.sum(loo_dense(K, noise, y, mean)[2]))


def tolerance(case, ref, K=None):
    """Per component of `ref` (see the module docstring).  `case`: kind, cond, weak, logNoise (+ y, mean and K for the
    weak-signal IsoLinear floor)."""
    tol = np.full(ref.size, max(1e-13, 64.0 * float(case["cond"]) * EPS * max(1.0, float(np.max(np.abs(ref))))))
    if case["weak"] and int(case["kind"]) == 2:
        noise = float(np.exp(2.0 * case["logNoise"]))
        _, (G, d, alpha, u, w) = loo_matrix(K, noise, case["y"], case["mean"])
        H2 = float(np.sum((G * np.sqrt(w)) ** 2))
        halves = float(np.sum(alpha * alpha / d) + np.sum(w * d) + (noise + JITTER) * (abs(u @ alpha) + H2))
        tol[0] += 8.0 * EPS * halves
    return tol
