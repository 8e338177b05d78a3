"""Dense float64 input gradients of the predictive means of several target columns on one leaf, and their tolerances: column q
is predgrad_dense.moments on Y[:, q] with mean[q] -- the same factor for every column -- and predgrad_dense.tolerances with
y = Y[:, q] (the project's RTOL / ATOL; nothing new)."""
import numpy as np

import predgrad_dense as pgd


def moments(kind, loghyp, logNoise, X, Y, mean, Xt, L=None):
    """(mu[n_t, Q], var[n_t], dmu[n_t, D, Q], dvar[n_t, D]) of one leaf: the variance and its gradient do not depend on the
    column.  `L` (lower factor of K_y) may be given (the device's own, `Context.download_factor`)."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (Y.shape[1],))
    cols = [pgd.moments(kind, loghyp, logNoise, X, Y[:, q], float(mean[q]), Xt, L=L) for q in range(Y.shape[1])]
    return (np.stack([c[0] for c in cols], axis=1), cols[0][1], np.stack([c[2] for c in cols], axis=2), cols[0][3])


def tolerances(kind, loghyp, logNoise, X, Y, Xt, dmu):
    """tol[n_t, D, Q] for dmu[n_t, D, Q]: per column predgrad_dense.tolerances with y = Y[:, q]."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    return np.stack([pgd.tolerances(kind, loghyp, logNoise, X, Y[:, q], Xt, dmu[:, :, q], np.zeros(dmu.shape[:2]))[0]
                     for q in range(Y.shape[1])], axis=2)
