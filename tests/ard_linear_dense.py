"""Dense NumPy / SciPy restatement of one GP leaf with the ArdLinear kernel (include/dsmgp_hip.h, DSMGP_KIND_ARD_LINEAR).

oracle/ has no ArdLinear: the reference's own cannot be fitted (src/kernels.jl:232,247), so the repaired kernel is restated
here -- k(a, b) = sum_d a_d b_d / l_d^2 -- with the GP arithmetic of oracle/gp.py (src/gaussianprocess.jl:82-137,163) and the
length-scale gradients in closed form.  It mirrors oracle.gp.GaussianProcess's interface (mll, prediction, grad), so the tree
recursions of oracle/spn.py run on it, and with all l_d equal it reproduces oracle.gp's IsoLinear
(tests/test_ard_linear_host.py)."""
import numpy as np
import scipy.linalg as sla

EPS = 1e-8  # src/DeepStructuredMixtures.jl:27


def kernelmatrix(logl, x1, x2):
    """sum_d (a_d b_d) / l_d^2, dimensions added in ascending order."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    s = 1.0 / np.exp(np.asarray(logl, dtype=np.float64)) ** 2
    K = np.zeros((x1.shape[0], x2.shape[0]))
    for d in range(x1.shape[1]):
        K += np.outer(x1[:, d], x2[:, d]) * s[d]
    return K


def prior_diag(logl, x):
    x = np.asarray(x, dtype=np.float64)
    return (x * x) @ (1.0 / np.exp(np.asarray(logl, dtype=np.float64)) ** 2)


class DenseGP:
    def __init__(self, x, y, mean, logl, logNoise):
        self.x = np.asarray(x, dtype=np.float64)
        self.N, self.D = self.x.shape
        self.mean = float(mean)
        self.y = np.asarray(y, dtype=np.float64) - self.mean
        self.logl = np.asarray(logl, dtype=np.float64).reshape(-1)
        self.logNoise = float(logNoise)
        self.noise = np.exp(2.0 * self.logNoise)
        Ky = kernelmatrix(self.logl, self.x, self.x)
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
        Knt = kernelmatrix(self.logl, self.x, xt)
        mu = self.mean + Knt.T @ self.alpha
        V = sla.solve_triangular(self.Lf, Knt, lower=True)
        return mu, prior_diag(self.logl, xt) - np.sum(V * V, axis=0) + self.noise

    def quad_terms(self):
        """(alpha . x_d)^2 and x_d^T K_y^-1 x_d per dimension."""
        W = sla.solve_triangular(self.Lf, self.x, lower=True)
        return (self.alpha @ self.x) ** 2, np.sum(W * W, axis=0)

    def grad(self):
        """[dl_1..dl_D, 0, dnoise]: dl_d = 0.5 tr((alpha alpha^T - K_y^-1) dK/dlog l_d) = -(A_d - Q_d) / l_d^2."""
        A, Q = self.quad_terms()
        dl = -(A - Q) / np.exp(self.logl) ** 2
        trKinv = np.sum(sla.solve_triangular(self.Lf, np.eye(self.N), lower=True) ** 2)
        dnoise = self.noise * (np.dot(self.alpha, self.alpha) - trKinv)
        return np.concatenate([dl, [0.0, dnoise]])
