"""Dense NumPy / SciPy restatement of one GP leaf with the ArdSEProduct kernel (include/dsmgp_hip.h, DSMGP_KIND_ARD_SE_PRODUCT).

oracle/ has no product-form ARD kernel (the reference's ArdSE is additive, src/kernels.jl:39-49), so it is restated here --
k(a, b) = sigma^2 exp(-0.5 sum_d (a_d - b_d)^2 / l_d^2) -- with the GP arithmetic of oracle/gp.py (src/gaussianprocess.jl:82-137,163)
and every gradient as the direct trace 0.5 tr(W dK/dtheta), W = alpha alpha^T - K_y^-1.  It mirrors oracle.gp.GaussianProcess's
interface (mll, prediction, grad), so the tree recursions of oracle/spn.py run on it."""
import numpy as np
import scipy.linalg as sla

EPS = 1e-8  # src/DeepStructuredMixtures.jl:27


def sqdist(x1, x2):
    """Per-dimension squared differences, shape (D, n1, n2)."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    return np.stack([(x1[:, d][:, None] - x2[:, d][None, :]) ** 2 for d in range(x1.shape[1])])


def exponent(logl, x1, x2):
    """z = sum_d (a_d - b_d)^2 * (-0.5 / l_d^2), dimensions added in ascending order."""
    nh = -0.5 / np.exp(np.asarray(logl, dtype=np.float64)) ** 2
    U = sqdist(x1, x2)
    z = np.zeros(U.shape[1:])
    for d in range(U.shape[0]):
        z += U[d] * nh[d]
    return z


def kernelmatrix(logl, logs, x1, x2):
    return np.exp(2.0 * float(logs)) * np.exp(exponent(logl, x1, x2))


class DenseGP:
    def __init__(self, x, y, mean, logl, logs, logNoise):
        self.x = np.asarray(x, dtype=np.float64)
        self.N, self.D = self.x.shape
        self.mean = float(mean)
        self.y = np.asarray(y, dtype=np.float64) - self.mean
        self.logl = np.asarray(logl, dtype=np.float64).reshape(-1)
        self.logs = float(logs)
        self.logNoise = float(logNoise)
        self.noise = np.exp(2.0 * self.logNoise)
        self.K = kernelmatrix(self.logl, self.logs, self.x, self.x)
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

    def prediction(self, xtest):
        xt = np.asarray(xtest, dtype=np.float64)
        Knt = kernelmatrix(self.logl, self.logs, self.x, xt)
        mu = self.mean + Knt.T @ self.alpha
        V = sla.solve_triangular(self.Lf, Knt, lower=True)
        return mu, np.exp(2.0 * self.logs) - np.sum(V * V, axis=0) + self.noise

    def grad(self):
        """[dl_1..dl_D, ds, dnoise], each 0.5 tr(W dK/dtheta): dK/dlog l_d = K o U_d / l_d^2, dK/dlog s = 2 K, dK_y/dlog sn = 2 noise I."""
        Linv = sla.solve_triangular(self.Lf, np.eye(self.N), lower=True)
        W = np.outer(self.alpha, self.alpha) - Linv.T @ Linv
        WK = W * self.K
        U = sqdist(self.x, self.x)
        il2 = 1.0 / np.exp(self.logl) ** 2
        dl = np.array([0.5 * np.sum(WK * U[d]) * il2[d] for d in range(self.D)])
        return np.concatenate([dl, [np.sum(WK), self.noise * np.trace(W)]])
