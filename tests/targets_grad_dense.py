"""Float64 dense reference for the hyper-parameter gradients of the per-column log marginal likelihoods of several target
columns on one factorisation (dsmgp_mll_columns_gradients), and the tolerance of its tests.

`column_gradients(kind, hyp, X, Y, mean)` restates, for every column j of Y, the gradient of
    mll_j = -((y_j - m_j)' K_y^-1 (y_j - m_j) + log det K_y + n log 2pi) / 2,      K_y = K + (noise + 1e-8) I,
in the library's convention (include/dsmgp_hip.h at dsmgp_gradients: [dl..., ds, dnoise], [dl..., da, ds, dnoise] for the
rational quadratic kinds; the reference's factor sigma on both IsoSE slots and on the ArdSE variance slot; ArdSE dl zero
unless `ard_true`; IsoLinear dl = 0.5 tr(P (-2K)) and a zero dummy slot; ArdLinear's true dl and a zero dummy slot; the true
derivatives for ArdSEProduct, Matern and rational quadratic) straight from the textbook equation
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
import os

import numpy as np
import scipy.linalg as sla

EPS = np.finfo(np.float64).eps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

ARD_KINDS = (1, 3, 4, 7, 8, 10)
RQ_KINDS = (9, 10)


def n_hyper(kind, D):
    """Length of the library hyper-vector including logNoise."""
    return (D if kind in ARD_KINDS else 1) + (1 if kind in RQ_KINDS else 0) + 2


def load_cases():
    z = np.load(os.path.join(GOLDEN, "gp_targets_grad.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = z[key]
    return cases


def kernel_and_derivatives(kind, h, X):
    """(K, [dK / dtheta for the slots before logNoise, in the library's order and convention]) in float64; `h` without the noise.
    For ArdSE the length-scale slots hold the TRUE derivatives (the caller zeroes them when the option is off)."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    ard = kind in ARD_KINDS
    nl = D if ard else 1
    il2 = np.exp(-2.0 * np.asarray(h[:nl], dtype=np.float64))
    il2 = il2 if ard else np.repeat(il2, D)
    U2 = (X[:, None, :] - X[None, :, :]) ** 2            # n x n x D
    Q = U2 * il2[None, None, :]                           # u_d^2 / l_d^2
    zero = np.zeros((n, n))
    if kind in (2, 3):
        if kind == 2:
            K = (X @ X.T) * il2[0]
            return K, [-2.0 * K, zero]
        K = (X * il2[None, :]) @ X.T
        return K, [-2.0 * np.outer(X[:, d], X[:, d]) * il2[d] for d in range(D)] + [zero]
    if kind in RQ_KINDS:
        al, s2 = np.exp(h[nl]), np.exp(2.0 * h[nl + 1])
        w = Q.sum(axis=2) / (2.0 * al)
        K = s2 * np.exp(-al * np.log1p(w))
        per = [K / (1.0 + w) * Q[:, :, d] for d in range(D)]
        dl = per if ard else [sum(per)]
        return K, dl + [K * al * (w / (1.0 + w) - np.log1p(w)), 2.0 * K]
    s2 = np.exp(2.0 * h[nl])
    sigma = np.exp(h[nl])
    if kind == 1:
        E = s2 * np.exp(-0.5 * Q)
        K = E.sum(axis=2)
        return K, [E[:, :, d] * Q[:, :, d] for d in range(D)] + [sigma * 2.0 * K]
    r2 = Q.sum(axis=2)
    if kind == 0:
        K = s2 * np.exp(-0.5 * r2)
        return K, [sigma * K * r2, sigma * 2.0 * K]
    if kind == 4:
        K = s2 * np.exp(-0.5 * r2)
        return K, [K * Q[:, :, d] for d in range(D)] + [2.0 * K]
    nu2 = 3.0 if kind in (5, 7) else 5.0
    s = np.sqrt(nu2 * r2)
    K = s2 * np.exp(-s) * (1.0 + s + (s * s / 3.0 if nu2 == 5.0 else 0.0))
    c = 1.0 if nu2 == 3.0 else (1.0 + s) / 3.0
    per = [s2 * np.exp(-s) * c * nu2 * Q[:, :, d] for d in range(D)]
    return K, (per if ard else [sum(per)]) + [2.0 * K]


def column_gradients(kind, hyp, X, Y, mean, ard_true=False):
    """(G[Q, len(hyp)], mll[Q], cond_2(K_y)): the gradient row and the log marginal of every column."""
    hyp = np.asarray(hyp, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    n, D = np.asarray(X).shape
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (Y.shape[1],))
    K, dK = kernel_and_derivatives(kind, hyp[:-1], X)
    noise = np.exp(2.0 * hyp[-1])
    Ky = K + (noise + 1e-8) * np.eye(n)
    F = sla.cholesky(Ky, lower=True)
    Kinv = sla.cho_solve((F, True), np.eye(n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    ev = np.linalg.eigvalsh(Ky)
    A = Kinv @ (Y - mean[None, :])
    logdet = 2.0 * np.sum(np.log(np.diag(F)))
    G = np.zeros((Y.shape[1], hyp.size))
    mll = np.zeros(Y.shape[1])
    for j in range(Y.shape[1]):
        a = A[:, j]
        P = np.outer(a, a) - Kinv
        for t, M in enumerate(dK):
            G[j, t] = 0.5 * np.sum(P * M)
        G[j, -1] = noise * np.trace(P)
        mll[j] = -(np.dot(Y[:, j] - mean[j], a) + logdet + n * np.log(2.0 * np.pi)) / 2.0
    if kind == 1 and not ard_true:
        G[:, :D] = 0.0
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
