"""Dense NumPy / SciPy restatement of one GP leaf with a Matern kernel (include/dsmgp_hip.h, DSMGP_KIND_*_MATERN*, kinds 5-8).

oracle/ has no Matern kernel (the reference has none), so it is restated here in the distance form of GPML's covMaterniso /
covMaternard -- r^2 = sum_d (a_d - b_d)^2 / l_d^2, s = sqrt(2 nu) r, k = sigma^2 (1 + s) e^-s (nu = 3/2) or
sigma^2 (1 + s + s^2 / 3) e^-s (nu = 5/2) -- with the GP arithmetic of oracle/gp.py (src/gaussianprocess.jl:82-137,163) and
every gradient as the direct trace 0.5 tr(W dK/dtheta), W = alpha alpha^T - K_y^-1, with
dK/dlog l_d = sigma^2 e^-s c(s) s_d^2, s_d^2 = 2 nu (a_d - b_d)^2 / l_d^2, c = 1 (nu = 3/2) or (1 + s) / 3 (nu = 5/2).
An iso kind has one l; its dl is the sum over d.  It mirrors oracle.gp.GaussianProcess's interface (mll, prediction, grad), so
the tree recursions of oracle/spn.py run on it."""
import numpy as np
import scipy.linalg as sla

EPS = 1e-8  # src/DeepStructuredMixtures.jl:27

ISO_MATERN32, ISO_MATERN52, ARD_MATERN32, ARD_MATERN52 = 5, 6, 7, 8
KINDS = (ISO_MATERN32, ISO_MATERN52, ARD_MATERN32, ARD_MATERN52)
NAMES = {ISO_MATERN32: "IsoMatern32", ISO_MATERN52: "IsoMatern52", ARD_MATERN32: "ArdMatern32", ARD_MATERN52: "ArdMatern52"}


def two_nu(kind):
    return 3.0 if kind in (ISO_MATERN32, ARD_MATERN32) else 5.0


def is_ard(kind):
    return kind in (ARD_MATERN32, ARD_MATERN52)


def sqdist(x1, x2):
    """Per-dimension squared differences, shape (D, n1, n2)."""
    x1 = np.asarray(x1, dtype=np.float64)
    x2 = np.asarray(x2, dtype=np.float64)
    return np.stack([(x1[:, d][:, None] - x2[:, d][None, :]) ** 2 for d in range(x1.shape[1])])


def factors(kind, logl, D):
    """2 nu / l_d^2 per dimension (an iso kind: D copies of its one factor)."""
    logl = np.asarray(logl, dtype=np.float64).reshape(-1)
    l2 = np.exp(logl) ** 2
    nh = two_nu(kind) / l2
    return nh if is_ard(kind) else np.full(D, nh[0])


def s2(kind, logl, x1, x2):
    """z = s^2 = sum_d (a_d - b_d)^2 * 2 nu / l_d^2, dimensions added in ascending order."""
    U = sqdist(x1, x2)
    nh = factors(kind, logl, U.shape[0])
    z = np.zeros(U.shape[1:])
    for d in range(U.shape[0]):
        z += U[d] * nh[d]
    return z


def poly(kind, s):
    return 1.0 + s if two_nu(kind) == 3.0 else 1.0 + s + s * s / 3.0


def kernelmatrix(kind, logl, logs, x1, x2):
    s = np.sqrt(s2(kind, logl, x1, x2))
    return np.exp(2.0 * float(logs)) * np.exp(-s) * poly(kind, s)


class DenseGP:
    def __init__(self, x, y, mean, kind, logl, logs, logNoise):
        self.x = np.asarray(x, dtype=np.float64)
        self.N, self.D = self.x.shape
        self.kind = int(kind)
        self.mean = float(mean)
        self.y = np.asarray(y, dtype=np.float64) - self.mean
        self.logl = np.asarray(logl, dtype=np.float64).reshape(-1)
        self.logs = float(logs)
        self.logNoise = float(logNoise)
        self.noise = np.exp(2.0 * self.logNoise)
        self.K = kernelmatrix(self.kind, self.logl, self.logs, self.x, self.x)
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
        Knt = kernelmatrix(self.kind, self.logl, self.logs, self.x, xt)
        mu = self.mean + Knt.T @ self.alpha
        V = sla.solve_triangular(self.Lf, Knt, lower=True)
        return mu, np.exp(2.0 * self.logs) - np.sum(V * V, axis=0) + self.noise

    def grad(self):
        """Iso [dl, ds, dnoise], ARD [dl_1..dl_D, ds, dnoise], each 0.5 tr(W dK/dtheta): dK/dlog l_d = sigma^2 e^-s c(s) s_d^2,
        dK/dlog s = 2 K, dK_y/dlog sn = 2 noise I."""
        Linv = sla.solve_triangular(self.Lf, np.eye(self.N), lower=True)
        W = np.outer(self.alpha, self.alpha) - Linv.T @ Linv
        s = np.sqrt(s2(self.kind, self.logl, self.x, self.x))
        c = np.ones_like(s) if two_nu(self.kind) == 3.0 else (1.0 + s) / 3.0
        Wg = W * (np.exp(2.0 * self.logs) * np.exp(-s) * c)
        U = sqdist(self.x, self.x)
        nh = factors(self.kind, self.logl, self.D)
        dl = np.array([0.5 * np.sum(Wg * U[d]) * nh[d] for d in range(self.D)])
        if not is_ard(self.kind):
            dl = np.array([np.sum(dl)])
        return np.concatenate([dl, [np.sum(W * self.K), self.noise * np.trace(W)]])
