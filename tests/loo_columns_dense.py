"""Float64 dense restatement of the leave-one-out moments and gradients of several target columns on one factorisation
(dsmgp_loo_columns, dsmgp_loo_columns_gradients; GPML 5.4.2, eqs. 5.10-5.13 per column), in two forms, and the tolerances of
their tests.

With K_y = K + (exp(2 logNoise) + 1e-8) I, G = K_y^-1, d = diag G and a_q = G (y_q - m_q) for column q, means held fixed:

    moments:  mu_iq = y_iq - a_iq / d_i,  var_i = 1 / d_i,  lpd_q = sum_i -(log 2pi - log d_i + a_iq^2 / d_i) / 2
    literal (5.13), per column:  dlpd_q/dtheta = sum_i (a_iq [Z a_q]_i - (1 + a_iq^2 / d_i) [Z G]_ii / 2) / d_i,  Z = G dK_y/dtheta
    M form, weights c_q >= 0:    sum_q c_q dlpd_q/dtheta = sum_rc M_rc (dK_y/dtheta)_rc,
                                 M = sum_q c_q (u_q a_q' + a_q u_q') / 2 - G diag(W) G,  u_q = G (a_q / d),
                                 W_i = (sum_q c_q + sum_q c_q a_iq^2 / d_i) / (2 d_i)

Every gradient component is the TRUE derivative for all eleven kinds of include/dsmgp_hip.h, as dsmgp_loo_gradients defines
them (dense_kernels.d_hyper: no factor sigma anywhere; the dummy variance slot of the linear kinds is zero).  `hyp` is the library
hyper-vector INCLUDING logNoise; gradients come back as [dl..., (da,) ds, dnoise].

Tolerances, the project's own rules and no new constants: the moments of column q get loo_dense.loo_tol of that column; the
weighted gradient gets loo_grad_dense.tolerance per column carried through the weighted sum, sum_q c_q tol_q, as
targets_grad_dense.tolerance does, including the weak-signal IsoLinear floor.  Against the 50-digit fixture they are used as
they are; where both sides are float64 the tests double them."""
import numpy as np
import scipy.linalg as sla

import dense_gp
import dense_kernels as dk
import loo_dense as ld
import loo_grad_dense as lgd
import targets_grad_dense as tgd

EPS = np.finfo(np.float64).eps
JITTER = dk.JITTER


def load_cases():
    cases = dk.load_cases("gp_loo_columns.npz")
    for c in cases.values():
        for f in ("kind", "n"):
            c[f] = int(c[f])
        c["weak"] = bool(c["weak"])
        c["cond"] = float(c["cond"])
    return cases


def _parts(kind, hyp, X, Y, mean):
    """K, dK_y/dtheta over all of hyp, noise, G = K_y^-1 formed explicitly, d, A = G (Y - mean), Y."""
    hyp = np.asarray(hyp, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y[:, None] if Y.ndim == 1 else Y
    n = Y.shape[0]
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (Y.shape[1],))
    K, dK = dk.d_hyper(kind, hyp[:-1], X)
    noise = float(np.exp(2.0 * hyp[-1]))
    G = sla.cho_solve((dense_gp.factor(K, noise), True), np.eye(n))
    G = 0.5 * (G + G.T)
    return K, dK + [2.0 * noise * np.eye(n)], noise, G, np.diag(G).copy(), G @ (Y - mean[None, :]), Y


def moments(kind, hyp, X, Y, mean):
    """(mu[n, Q], var[n], lpd[Q])."""
    _, _, _, _, d, A, Y = _parts(kind, hyp, X, Y, mean)
    mu = Y - A / d[:, None]
    lpd = np.sum(-0.5 * ((ld.LOG2PI - np.log(d))[:, None] + A * A / d[:, None]), axis=0)
    return mu, 1.0 / d, lpd


def column_gradients_literal(kind, hyp, X, Y, mean):
    """G[Q, len(hyp)]: GPML eq. 5.13 as printed, column by column."""
    _, dKy, _, G, d, A, _ = _parts(kind, hyp, X, Y, mean)
    out = np.zeros((A.shape[1], len(dKy)))
    for t, dK in enumerate(dKy):
        Z = G @ dK
        zg = np.diag(Z @ G)
        for q in range(A.shape[1]):
            a = A[:, q]
            out[q, t] = float(np.sum((a * (Z @ a) - 0.5 * (1.0 + a * a / d) * zg) / d))
    return out


def weighted_matrix(G, d, A, c):
    """M of the M form and (U, W)."""
    c = np.asarray(c, dtype=np.float64)
    U = G @ (A / d[:, None])
    W = (np.sum(c) + (A * A / d[:, None]) @ c) / (2.0 * d)
    UA = (U * c[None, :]) @ A.T
    return 0.5 * (UA + UA.T) - (G * W) @ G, U, W


def weighted_gradient(kind, hyp, X, Y, mean, c):
    """sum_q c_q dlpd_q/dtheta by the M form, one M for all columns."""
    _, dKy, _, G, d, A, _ = _parts(kind, hyp, X, Y, mean)
    M, _, _ = weighted_matrix(G, d, A, c)
    return np.array([float(np.sum(M * dK)) for dK in dKy])


def weighted(Gc, c):
    """sum_q c_q Gc[q] with the columns added in ascending q."""
    return tgd.weighted(Gc, c)


def moment_tolerances(case, q):
    """loo_dense.loo_tol of column q of a fixture case: (tol mu, tol var, tol lpd_i, tol of the column's sum)."""
    noise = float(np.exp(2.0 * case["hyp"][-1]))
    return ld.loo_tol(case["Y"][:, q], case["mu"][:, q], case["var"], case["kss"], noise)


def gradient_tolerance(case, Gc, c, K=None):
    """sum_q c_q loo_grad_dense.tolerance(column q): `Gc` the per-column reference gradients, `c` the weights."""
    if K is None:
        K = dk.d_hyper(case["kind"], case["hyp"][:-1], case["X"])[0]
    tol = np.zeros(Gc.shape[1])
    for q in range(Gc.shape[0]):
        col = dict(kind=case["kind"], cond=case["cond"], weak=case["weak"], logNoise=float(case["hyp"][-1]), y=case["Y"][:, q],
                   mean=float(case["mean"][q]))
        tol += abs(float(c[q])) * lgd.tolerance(col, Gc[q], K)
    return tol


def weights(Q):
    """The fixed non-negative weight vector of the fixture: 1.25 for one column; a zero at column 1 otherwise."""
    if Q == 1:
        return np.array([1.25])
    w = np.array([0.5 + 0.75 * (q % 4) for q in range(Q)])
    w[1] = 0.0
    return w
