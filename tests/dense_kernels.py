"""The eleven kernel kinds of include/dsmgp_hip.h in dense NumPy float64, once: values, true derivatives with respect to the
hyper-parameters and to the input, the prior diagonal, and the convention dsmgp_gradients puts on top of the true derivatives.
Every dense oracle under tests/ takes its kernel from here; nothing here imports the package under test or oracle/.

`h` is the library hyper-vector without the noise: [logl (one, or one per dimension for the ARD kinds), (loga for the rational
quadratic kinds,) logs]; the variance slot of the linear kinds is a dummy.  With D_d = a_d - b_d and r^2 = sum_d D_d^2 / l_d^2:

    IsoSE 0, ArdSEProduct 4     k = sigma^2 exp(-r^2 / 2)
    ArdSE 1 (additive)          k = sigma^2 sum_d exp(-D_d^2 / (2 l_d^2))
    IsoLinear 2, ArdLinear 3    k = sum_d a_d b_d / l_d^2
    Matern 3/2: 5 iso, 7 ARD    k = sigma^2 (1 + s) exp(-s),            s = sqrt(3) r
    Matern 5/2: 6 iso, 8 ARD    k = sigma^2 (1 + s + s^2 / 3) exp(-s),  s = sqrt(5) r
    RQ: 9 iso, 10 ARD           k = sigma^2 (1 + w)^-alpha,             w = r^2 / (2 alpha), alpha = exp(loga)"""
import os

import numpy as np

ARD = (1, 3, 4, 7, 8, 10)
LINEAR = (2, 3)
MATERN = (5, 6, 7, 8)
RQ = (9, 10)
JITTER = 1e-8      # K_y = K + (noise + JITTER) I is the matrix every fit factorises


def n_hyper(kind, D, noise=True):
    """Length of the library hyper-vector, with or without logNoise."""
    return (D if kind in ARD else 1) + (1 if kind in RQ else 0) + 1 + (1 if noise else 0)


def pack(kind, logl, logs=0.0, loga=None, logNoise=None):
    """The library hyper-vector from its split pieces; logs is the dummy slot of a linear kind."""
    return np.concatenate([np.asarray(logl, dtype=np.float64).reshape(-1), [loga] if kind in RQ else [], [logs],
                           [] if logNoise is None else [logNoise]]).astype(np.float64)


def unpack(kind, h, D):
    """(1 / l_d^2 per dimension, alpha or None, sigma^2 (1 for the linear kinds))."""
    h = np.asarray(h, dtype=np.float64)
    nl = D if kind in ARD else 1
    il2 = np.exp(-2.0 * h[:nl]) * np.ones(D)
    alpha = float(np.exp(h[nl])) if kind in RQ else None
    s2 = 1.0 if kind in LINEAR else float(np.exp(2.0 * h[n_hyper(kind, D, noise=False) - 1]))
    return il2, alpha, s2


def noisy(K, noise):
    """K_y = K + (noise + JITTER) I."""
    return np.asarray(K, dtype=np.float64) + (noise + JITTER) * np.eye(len(K))


def load_cases(npz_name):
    """tests/golden/<npz_name> with keys "case/field" as {case: {field: array}}."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", npz_name))
    cases = {}
    for key in z.files:
        name, field = key.split("/", 1)
        cases.setdefault(name, {})[field] = z[key]
    return cases


def two_nu(kind):
    """2 nu of a Matern kind."""
    return 3.0 if kind in (5, 7) else 5.0


def _radial(kind, alpha, s2, r2):
    """(k, c) of a kind that is a function of r^2 alone, with dk/d(r^2) = -c / 2 (so dk/dlog l_d = c D_d^2 / l_d^2 and
    dk/da_d = -c D_d / l_d^2)."""
    if kind in (0, 4):
        k = s2 * np.exp(-0.5 * r2)
        return k, k
    if kind in RQ:
        w = r2 / (2.0 * alpha)
        k = s2 * np.exp(-alpha * np.log1p(w))
        return k, k / (1.0 + w)
    nu2 = two_nu(kind)
    s = np.sqrt(nu2 * r2)
    k = s2 * np.exp(-s) * (1.0 + s + (s * s / 3.0 if nu2 == 5.0 else 0.0))
    return k, s2 * np.exp(-s) * (1.0 if nu2 == 3.0 else (1.0 + s) / 3.0) * nu2


def scaled_sqdist(kind, h, A, B):
    """r^2 = sum_d (a_d - b_d)^2 / l_d^2, (len(A), len(B))."""
    A, B = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(B, dtype=np.float64))
    d = A[:, None, :] - B[None, :, :]
    return np.sum(d * d * unpack(kind, h, A.shape[1])[0], axis=2)


def value(kind, h, A, B):
    """k(a_r, b_c), (len(A), len(B))."""
    A, B = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(B, dtype=np.float64))
    il2, alpha, s2 = unpack(kind, h, A.shape[1])
    if kind in LINEAR:
        return (A * il2) @ B.T
    d = A[:, None, :] - B[None, :, :]
    if kind == 1:
        return s2 * np.sum(np.exp(-0.5 * d * d * il2), axis=2)
    return _radial(kind, alpha, s2, np.sum(d * d * il2, axis=2))[0]


def d_hyper(kind, h, X):
    """(K, [dK / dtheta for every slot of h]): every slot the TRUE derivative with respect to the logarithm it stores; the dummy
    variance slot of the linear kinds is a zero matrix."""
    X = np.asarray(X, dtype=np.float64)
    n, D = X.shape
    il2, alpha, s2 = unpack(kind, h, D)
    if kind in LINEAR:
        K = value(kind, h, X, X)
        dl = [-2.0 * np.outer(X[:, d], X[:, d]) * il2[d] for d in range(D)] if kind == 3 else [-2.0 * K]
        return K, dl + [np.zeros((n, n))]
    Q = (X[:, None, :] - X[None, :, :]) ** 2 * il2          # D_d^2 / l_d^2
    if kind == 1:
        E = s2 * np.exp(-0.5 * Q)
        K = E.sum(axis=2)
        return K, [E[:, :, d] * Q[:, :, d] for d in range(D)] + [2.0 * K]
    r2 = Q.sum(axis=2)
    K, c = _radial(kind, alpha, s2, r2)
    if kind == 0:
        dl = [K * r2]
    else:
        dl = [c * Q[:, :, d] for d in range(D)]
        dl = dl if kind in ARD else [sum(dl)]
    if kind in RQ:
        w = r2 / (2.0 * alpha)
        dl = dl + [K * alpha * (w / (1.0 + w) - np.log1p(w))]
    return K, dl + [2.0 * K]


def mll_convention(kind, h, K, dK, ard_true=False):
    """The slots of `d_hyper` as dsmgp_gradients and dsmgp_mll_columns_gradients contract them: the reference's factor sigma on
    both IsoSE slots and on the ArdSE variance slot, and the ArdSE length-scale slots zero unless `ard_true`.  Every other slot
    is the true derivative."""
    if kind == 0:
        sigma = np.exp(h[1])
        return [sigma * dK[0], sigma * dK[1]]
    if kind == 1:
        return [M if ard_true else np.zeros_like(M) for M in dK[:-1]] + [np.exp(h[-1]) * dK[-1]]
    return list(dK)


def d_input(kind, h, Xt, X):
    """G[t, i, d] = dk(x_t, x_i) / dx_{t,d}: true derivatives, finite at x_t = x_i."""
    Xt, X = np.atleast_2d(np.asarray(Xt, dtype=np.float64)), np.atleast_2d(np.asarray(X, dtype=np.float64))
    il2, alpha, s2 = unpack(kind, h, X.shape[1])
    if kind in LINEAR:
        return np.broadcast_to((X * il2)[None, :, :], (Xt.shape[0],) + X.shape).copy()
    d = Xt[:, None, :] - X[None, :, :]
    if kind == 1:
        return -s2 * np.exp(-0.5 * d * d * il2) * d * il2
    c = _radial(kind, alpha, s2, np.sum(d * d * il2, axis=2))[1]
    return -c[:, :, None] * d * il2


def prior_diag(kind, h, Xt):
    """k(x, x) at the rows of Xt."""
    Xt = np.atleast_2d(np.asarray(Xt, dtype=np.float64))
    il2, _, s2 = unpack(kind, h, Xt.shape[1])
    if kind in LINEAR:
        return (Xt * Xt) @ il2
    return np.full(Xt.shape[0], s2 * (Xt.shape[1] if kind == 1 else 1.0))


def prior_dx(kind, h, Xt):
    """dk(x, x) / dx_d at the rows of Xt: 2 x_d / l_d^2 for the linear kinds, 0 for the stationary ones."""
    Xt = np.atleast_2d(np.asarray(Xt, dtype=np.float64))
    return 2.0 * Xt * unpack(kind, h, Xt.shape[1])[0] if kind in LINEAR else np.zeros(Xt.shape)


def grad_scale(kind, h, X, Xt):
    """g_d per (test row, dimension): the size of d/dx_d relative to the kernel's own scale -- 1 / l_d for the stationary kinds,
    max(1, max_i |x_{i,d}|, |x_{t,d}|) / l_d^2 relative to max(1, k**) for the linear ones."""
    X, Xt = np.atleast_2d(X), np.atleast_2d(Xt)
    il2 = unpack(kind, h, X.shape[1])[0]
    if kind not in LINEAR:
        return np.broadcast_to(np.sqrt(il2)[None, :], Xt.shape)
    big = np.maximum(np.maximum(1.0, np.max(np.abs(X), axis=0))[None, :], np.abs(Xt))
    return big * il2[None, :] / np.maximum(1.0, prior_diag(kind, h, Xt))[:, None]
