"""Float64 dense reference for the hyper-parameter gradients of the per-column log marginal likelihoods of several target
columns on one factorisation (dsmgp_mll_columns_gradients), and the tolerance of its tests.

`column_gradients(kind, hyp, X, Y, mean)` restates, for every column j of Y, the gradient of
    mll_j = -((y_j - m_j)' K_y^-1 (y_j - m_j) + log det K_y + n log 2pi) / 2,      K_y = K + (noise + 1e-8) I,
in the library's convention (include/dsmgp_hip.h at dsmgp_gradients: [dl..., ds, dnoise], [dl..., da, ds, dnoise] for the
rational quadratic kinds; the slots of dense_kernels.mll_convention) straight from the textbook equation
    d mll_j / d theta = 0.5 tr((alpha_j alpha_j' - K_y^-1) dK_y / d theta),   alpha_j = K_y^-1 (y_j - m_j),
with K_y^-1 formed explicitly from SciPy's Cholesky factor -- not by the device's route (L^-T arena, a rank-Q update of the
contraction's accumulators, the trace identity for the variance slot).  `hyp` is the library hyper-vector INCLUDING logNoise.

Tolerance: the project's rule for a gradient component (tests/test_gradients_gpu._tolerance), applied per column and carried
through the weighted sum:
    tol = sum_j |w_j| max(1e-13, 64 cond_2(K_y) eps max(1, |g_j|_inf)),
plus, for weak-signal cases, sum_j |w_j| times the floor of the trace identity the host uses for tr(P K), 8 eps (n + c tr K_y^-1),
on the components it enters (IsoSE ds times sigma, IsoLinear dl).  Where BOTH sides are float64 (the device against this
module) each side rounds and the tests double it, as tests/test_targets_gpu.py does; against the 50-digit fixture it is used
as it is."""
import numpy as np
import scipy.linalg as sla

import dense_gp
import dense_kernels as dk

EPS = np.finfo(np.float64).eps


def load_cases():
    return dk.load_cases("gp_targets_grad.npz")


def gradients_from_factor(kind, hyp, X, F, Y, mean, ard_true=False, kernel=None):
    """(G[Q, len(hyp)], A = K_y^-1 (Y - mean)) from a lower factor F of K_y: K_y^-1 formed explicitly, then the textbook trace.
    `kernel`: dense_kernels.d_hyper of the leaf, where the caller has it."""
    hyp = np.asarray(hyp, dtype=np.float64)
    n = F.shape[0]
    K, dK = kernel or dk.d_hyper(kind, hyp[:-1], X)
    dK = dk.mll_convention(kind, hyp[:-1], K, dK, ard_true)
    noise = np.exp(2.0 * hyp[-1])
    Kinv = sla.cho_solve((F, True), np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    A = Kinv @ (Y - mean[None, :])
    G = np.zeros((Y.shape[1], hyp.size))
    for j in range(Y.shape[1]):
        P = np.outer(A[:, j], A[:, j]) - Kinv
        for t, M in enumerate(dK):
            G[j, t] = 0.5 * np.sum(P * M)
        G[j, -1] = noise * np.trace(P)
    return G, A


def column_gradients(kind, hyp, X, Y, mean, ard_true=False):
    """(G[Q, len(hyp)], mll[Q], cond_2(K_y)): the gradient row and the log marginal of every column."""
    hyp = np.asarray(hyp, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    n = Y.shape[0]
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (Y.shape[1],))
    K, dK = dk.d_hyper(kind, hyp[:-1], X)
    noise = np.exp(2.0 * hyp[-1])
    F = dense_gp.factor(K, noise)
    ev = np.linalg.eigvalsh(dk.noisy(K, noise))
    G, A = gradients_from_factor(kind, hyp, X, F, Y, mean, ard_true, kernel=(K, dK))
    logdet = 2.0 * np.sum(np.log(np.diag(F)))
    mll = np.array([-(np.dot(Y[:, j] - mean[j], A[:, j]) + logdet + n * np.log(2.0 * np.pi)) / 2.0 for j in range(Y.shape[1])])
    return G, mll, float(ev[-1] / ev[0])


def weighted(G, w):
    """sum_j w_j G[j] with the columns added in ascending j."""
    out = np.zeros(G.shape[1])
    for j in range(G.shape[0]):
        out += w[j] * G[j]
    return out


def tolerance(G, w, cond, kind=None, hyp=None, weak=False, n=0, c_trKinv=0.0):
    """Per component of sum_j w_j G[j] (module docstring); G are the per-column reference gradients."""
    G = np.asarray(G, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    per_col = np.maximum(1e-13, 64.0 * float(cond) * EPS * np.maximum(1.0, np.max(np.abs(G), axis=1)))
    tol = np.full(G.shape[1], float(np.sum(np.abs(w) * per_col)))
    if weak:
        floor = 8.0 * EPS * (float(n) + float(c_trKinv)) * float(np.sum(np.abs(w)))
        if int(kind) == 0:
            tol[1] += floor * np.exp(float(hyp[1]))
        elif int(kind) == 2:
            tol[0] += floor
    return tol


def signed_weights(Q):
    """The fixed signed weight vector of the fixture: alternating signs, magnitudes 0.5 .. 2.75, a zero at column 2."""
    w = np.array([(-1.0) ** j * (0.5 + 0.75 * (j % 4)) for j in range(Q)])
    if Q > 2:
        w[2] = 0.0
    return w
