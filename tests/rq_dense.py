"""Dense NumPy / SciPy restatement of one GP leaf with a rational quadratic kernel (include/dsmgp_hip.h, DSMGP_KIND_ISO_RQ /
DSMGP_KIND_ARD_RQ, kinds 9 and 10).

oracle/ has no rational quadratic kernel (the reference has none), so it is restated here as GPML's covRQiso / covRQard --
w = sum_d (a_d - b_d)^2 / (2 alpha l_d^2), k = sigma^2 (1 + w)^-alpha, alpha = exp(loga) -- with the GP arithmetic of
oracle/gp.py (src/gaussianprocess.jl:82-137,163).  Hyper-vector without the noise: [logl..., loga, logs].  Derivatives:
    dK/dlog l_d   = k / (1 + w) (a_d - b_d)^2 / l_d^2          (the iso kind's dl: the sum over d)
    dK/dlog alpha = k alpha (w / (1 + w) - log1p(w))
    dK/dlog sigma = 2 K,   dK_y/dlog sn = 2 noise I
    dk(x_t, x_i)/dx_{t,d} = -k / (1 + w) (x_{t,d} - x_{i,d}) / l_d^2
`DenseGP` mirrors oracle.gp.GaussianProcess's interface (mll, prediction, grad), so the tree recursions of oracle/spn.py run
on it; grad is the direct trace 0.5 tr(W dK/dtheta), W = alpha alpha^T - K_y^-1, in the order [dl..., da, ds, dnoise].
`loo` is the leave-one-out density of GPML 5.4.2 (eqs. 5.10-5.12), `loo_grad` its gradient (eq. 5.13) in the M form of the
header, `input_gradients` the derivatives of the predictive moments with respect to the test point."""
import os

import numpy as np
import scipy.linalg as sla

EPS = 1e-8  # src/DeepStructuredMixtures.jl:27

ISO_RQ, ARD_RQ = 9, 10
KINDS = (ISO_RQ, ARD_RQ)
NAMES = {ISO_RQ: "IsoRQ", ARD_RQ: "ArdRQ"}


def load_cases():
    """The cases of tests/golden/gp_rq.npz (tests/golden/make_rq_golden.py), name -> dict of arrays and Python scalars."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_rq.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        v = z[key]
        cases.setdefault(name, {})[field] = v if v.ndim else v.item()
    return cases


def is_ard(kind):
    return kind == ARD_RQ


def sqdist(x1, x2):
    """Per-dimension squared differences, shape (D, n1, n2)."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    return np.stack([(x1[:, d][:, None] - x2[:, d][None, :]) ** 2 for d in range(x1.shape[1])])


def factors(kind, logl, loga, D):
    """1 / (2 alpha l_d^2) per dimension (the iso kind: D copies of its one factor)."""
    logl = np.asarray(logl, dtype=np.float64).reshape(-1)
    l2 = np.exp(logl) ** 2
    nh = (0.5 / np.exp(float(loga))) / l2
    return nh if is_ard(kind) else np.full(D, nh[0])


def wsum(kind, logl, loga, x1, x2):
    """w = sum_d (a_d - b_d)^2 / (2 alpha l_d^2), dimensions added in ascending order."""
    U = sqdist(x1, x2)
    nh = factors(kind, logl, loga, U.shape[0])
    w = np.zeros(U.shape[1:])
    for d in range(U.shape[0]):
        w += U[d] * nh[d]
    return w


def kernelmatrix(kind, logl, loga, logs, x1, x2):
    w = wsum(kind, logl, loga, x1, x2)
    return np.exp(2.0 * float(logs)) * np.exp(-np.exp(float(loga)) * np.log1p(w))


class DenseGP:
    def __init__(self, x, y, mean, kind, logl, loga, logs, logNoise):
        self.x = np.asarray(x, dtype=np.float64)
        self.N, self.D = self.x.shape
        self.kind = int(kind)
        self.mean = float(mean)
        self.y = np.asarray(y, dtype=np.float64) - self.mean
        self.logl = np.asarray(logl, dtype=np.float64).reshape(-1)
        self.loga = float(loga)
        self.logs = float(logs)
        self.logNoise = float(logNoise)
        self.noise = np.exp(2.0 * self.logNoise)
        self.K = kernelmatrix(self.kind, self.logl, self.loga, self.logs, self.x, self.x)
        Ky = self.K.copy()
        Ky[np.diag_indices(self.N)] += self.noise + EPS
        C, info = sla.lapack.dpotrf(Ky, lower=1, clean=1)
        self.info = int(info)
        self.Lf = np.tril(C)
        self.alpha = sla.cho_solve((self.Lf, True), self.y)

    def L(self):
        return self.Lf

    def mll(self):
        logdet = 2.0 * np.sum(np.log(np.diag(self.Lf)))
        return -(np.dot(self.y, self.alpha) + logdet + np.log(2.0 * np.pi) * self.N) / 2.0

    def _k(self, xt):
        return kernelmatrix(self.kind, self.logl, self.loga, self.logs, self.x, xt)

    def prediction(self, xtest):
        xt = np.asarray(xtest, dtype=np.float64)
        Knt = self._k(xt)
        mu = self.mean + Knt.T @ self.alpha
        V = sla.solve_triangular(self.Lf, Knt, lower=True)
        return mu, np.exp(2.0 * self.logs) - np.sum(V * V, axis=0) + self.noise

    def prediction_cov(self, xtest, with_noise=True):
        xt = np.asarray(xtest, dtype=np.float64)
        V = sla.solve_triangular(self.Lf, self._k(xt), lower=True)
        S = kernelmatrix(self.kind, self.logl, self.loga, self.logs, xt, xt) - V.T @ V
        return S + (self.noise * np.eye(xt.shape[0]) if with_noise else 0.0)

    def kernel_derivatives(self):
        """[dK/dlog l..., dK/dlog alpha, dK/dlog sigma] in the order of the hyper-vector."""
        w = wsum(self.kind, self.logl, self.loga, self.x, self.x)
        a = np.exp(self.loga)
        q = 1.0 / (1.0 + w)
        U = sqdist(self.x, self.x)
        il2 = 2.0 * a * factors(self.kind, self.logl, self.loga, self.D)
        dl = [self.K * q * U[d] * il2[d] for d in range(self.D)]
        if not is_ard(self.kind):
            dl = [sum(dl)]
        return dl + [self.K * a * (w * q - np.log1p(w)), 2.0 * self.K]

    def _G(self):
        Linv = sla.solve_triangular(self.Lf, np.eye(self.N), lower=True)
        return Linv.T @ Linv

    def grad(self):
        """[dl..., da, ds, dnoise], each 0.5 tr(W dK_y/dtheta)."""
        W = np.outer(self.alpha, self.alpha) - self._G()
        g = [0.5 * np.sum(W * dK) for dK in self.kernel_derivatives()]
        return np.array(g + [self.noise * np.trace(W)])

    def loo(self):
        """(mu, var, lpd) of GPML eqs. 5.10-5.12 on K_y = K + (noise + 1e-8) I."""
        d = np.diag(self._G())
        var = 1.0 / d
        mu = (self.y + self.mean) - self.alpha / d
        lpd = np.sum(-(np.log(2.0 * np.pi) + np.log(var) + (self.alpha / d) ** 2 / var) / 2.0)
        return mu, var, lpd

    def loo_grad(self):
        """dlpd/dtheta = sum_rc M_rc (dK_y/dtheta)_rc, M = (u alpha' + alpha u') / 2 - G diag(w) G (eq. 5.13)."""
        G = self._G()
        d = np.diag(G)
        u = G @ (self.alpha / d)
        wv = (1.0 + self.alpha ** 2 / d) / (2.0 * d)
        M = 0.5 * (np.outer(u, self.alpha) + np.outer(self.alpha, u)) - (G * wv) @ G
        g = [np.sum(M * dK) for dK in self.kernel_derivatives()]
        return np.array(g + [2.0 * self.noise * np.trace(M)])

    def input_gradients(self, xtest):
        """(dmu, dvar), each (n_t, D): derivatives of `prediction` with respect to the test point; k(x, x) is constant."""
        xt = np.asarray(xtest, dtype=np.float64)
        Knt = self._k(xt)                                        # (N, n_t)
        w = wsum(self.kind, self.logl, self.loga, self.x, xt)
        il2 = 2.0 * np.exp(self.loga) * factors(self.kind, self.logl, self.loga, self.D)
        diff = xt[None, :, :] - self.x[:, None, :]               # (N, n_t, D): x_t - x_i
        dk = -(Knt / (1.0 + w))[:, :, None] * diff * il2
        beta = sla.cho_solve((self.Lf, True), Knt)               # (N, n_t)
        return np.einsum("i,itd->td", self.alpha, dk), -2.0 * np.einsum("it,itd->td", beta, dk)
