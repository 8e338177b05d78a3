"""One exact GP leaf in dense NumPy / SciPy float64, for every kernel kind of tests/dense_kernels.py: the reference the host and
device tests compare against, with oracle.gp.GaussianProcess's interface (L, mll, prediction, grad, info), so the tree
recursions of oracle/spn.py and the oracle contexts of tests/ run on it.

K_y = K + (noise + 1e-8) I = F F' is the matrix the fit factorises (`factor`, the one place that does); z = F^-1 (y - m),
alpha = F^-T z, G = K_y^-1 = F^-T F^-1.  `hyp` is the library hyper-vector INCLUDING logNoise.

    mll             -(|z|^2 + 2 sum log F_ii + n log 2pi) / 2
    prediction      mu = m + k_t . alpha,  var = k(x_t, x_t) - |F^-1 k_t|^2 + noise;  prediction_cov: the full matrix
    grad            0.5 tr((alpha alpha' - G) dK_y/dtheta) in the convention of dsmgp_gradients (dense_kernels.mll_convention)
    loo             GPML 5.4.2, eqs. 5.10-5.12: mu_i = y_i - alpha_i / G_ii, var_i = 1 / G_ii, and the sum of the log densities
    loo_grad        its gradient (eq. 5.13) in the M form, sum_rc M_rc (dK_y/dtheta)_rc, on the TRUE derivatives
    input_gradients d mu / d x_t and d var / d x_t
Gradients come back as [dl..., (da,) ds, dnoise].  A matrix that is not positive definite gives info = 1, the unit factor and NaN
z, alpha and mll."""
import numpy as np
import scipy.linalg as sla

import dense_kernels as dk

LOG2PI = float(np.log(2.0 * np.pi))


def factor(K, noise):
    """The lower Cholesky factor of K_y = K + (noise + 1e-8) I; raises (LinAlgError, ValueError) where there is none."""
    return sla.cholesky(dk.noisy(K, noise), lower=True)


class DenseGP:
    def __init__(self, kind, hyp, X, y, mean, F=None, alpha=None):
        """`F` (a lower factor of K_y) and `alpha` may be given -- a device's own, Context.download_factor -- in place of SciPy's."""
        self.kind, self.hyp, self.mean = int(kind), np.asarray(hyp, dtype=np.float64), float(mean)
        self.x, self.y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self.N, self.D = self.x.shape
        self.h, self.logNoise, self.noise = self.hyp[:-1], float(self.hyp[-1]), float(np.exp(2.0 * self.hyp[-1]))
        self.K = dk.value(self.kind, self.h, self.x, self.x)
        self.info, self._cond = 0, None
        try:
            self.F = factor(self.K, self.noise) if F is None else np.tril(np.asarray(F, dtype=np.float64))
            self.z = sla.solve_triangular(self.F, self.y - self.mean, lower=True)
            self.alpha = sla.solve_triangular(self.F, self.z, lower=True, trans="T") if alpha is None else np.asarray(alpha)
        except (sla.LinAlgError, ValueError):
            self.F, self.info, self._cond = np.eye(self.N), 1, float("inf")
            self.z = self.alpha = np.full(self.N, np.nan)

    @property
    def cond(self):
        """cond_2(K_y)."""
        if self._cond is None:
            ev = np.linalg.eigvalsh(dk.noisy(self.K, self.noise))
            self._cond = float(ev[-1] / ev[0])
        return self._cond

    def L(self):
        return self.F

    def G(self):
        Finv = sla.solve_triangular(self.F, np.eye(self.N), lower=True)
        return Finv.T @ Finv

    def mll(self):
        if self.info:
            return float("nan")
        return float(-(self.z @ self.z + 2.0 * np.sum(np.log(np.diag(self.F))) + LOG2PI * self.N) / 2.0)

    def _cross(self, Xt):
        Ktn = dk.value(self.kind, self.h, Xt, self.x)
        return Ktn, sla.solve_triangular(self.F, Ktn.T, lower=True)        # V = F^-1 k_t, n x n_t

    def prediction(self, Xt):
        Ktn, V = self._cross(Xt)
        return self.mean + Ktn @ self.alpha, dk.prior_diag(self.kind, self.h, Xt) - np.sum(V * V, axis=0) + self.noise

    def prediction_cov(self, Xt, with_noise=True):
        V = self._cross(Xt)[1]
        S = dk.value(self.kind, self.h, Xt, Xt) - V.T @ V
        return S + (self.noise * np.eye(S.shape[0]) if with_noise else 0.0)

    def input_gradients(self, Xt):
        """(dmu, dvar), each (n_t, D)."""
        V = self._cross(Xt)[1]
        beta = sla.solve_triangular(self.F, V, lower=True, trans="T").T      # n_t x n
        Gx = dk.d_input(self.kind, self.h, Xt, self.x)
        return np.einsum("i,tid->td", self.alpha, Gx), dk.prior_dx(self.kind, self.h, Xt) - 2.0 * np.einsum("ti,tid->td", beta, Gx)

    def _dKy(self):
        return dk.d_hyper(self.kind, self.h, self.x)[1], 2.0 * self.noise * np.eye(self.N)

    def grad(self, ard_true=False):
        dK, dn = self._dKy()
        W = np.outer(self.alpha, self.alpha) - self.G()
        return np.array([0.5 * np.sum(W * M) for M in dk.mll_convention(self.kind, self.h, self.K, dK, ard_true) + [dn]])

    def loo(self):
        """(mu, var, sum_i lpd_i)."""
        d = np.diag(self.G())
        mu, var = self.y - self.alpha / d, 1.0 / d
        return mu, var, float(np.sum(-(LOG2PI + np.log(var) + (self.y - mu) ** 2 / var) / 2.0))

    def loo_grad(self):
        G = self.G()
        d = np.diag(G)
        u = G @ (self.alpha / d)
        w = (1.0 + self.alpha ** 2 / d) / (2.0 * d)
        M = 0.5 * (np.outer(u, self.alpha) + np.outer(self.alpha, u)) - (G * w) @ G
        dK, dn = self._dKy()
        return np.array([np.sum(M * dM) for dM in dK + [dn]])

    def quad_terms(self):
        """(alpha . x_d)^2 and x_d' K_y^-1 x_d per dimension: the two halves of a linear kind's dl_d = -(A_d - Q_d) / l_d^2."""
        W = sla.solve_triangular(self.F, self.x, lower=True)
        return (self.alpha @ self.x) ** 2, np.sum(W * W, axis=0)
