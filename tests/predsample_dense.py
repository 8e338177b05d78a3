"""Dense float64 side of the tests of dsmgp_predict_sample: the bounds of tests/test_predsample_gpu.py, written once, and a
test double that answers predict_sample / predict_cov_factor with NumPy so that the CPU suite drives the host composition
(model.posterior_sample(device=True), leaf_samples, mixture_sample) without a GPU.  Nothing here reads the library.

Bounds (u = 2^-53, gamma_m = m u / (1 - m u); Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.):
  * the factor: ||A - C C'||_F <= 4e-15 ||A||_F, the project's criterion for its training factor (test_cholesky_backward_error);
  * a draw against the device's own factor: |out - (mu + C eps)|_i <= 2 gamma_{nt+2} (sum_j |C_ij| |eps_js| + |mu_i|): the inner
    product bound of any summation order (ASNA (3.5)) with the final addition, doubled because the reference is float64 too;
  * a draw against another Cholesky of the same matrix (LAPACK): with eps_f = ||A - C C'||_F / ||A||_2 of a factor, both factors
    are exact factors of perturbations of A, and Sun's bound (ASNA Theorem 10.8) gives
        ||C_dev - C_host||_F <= ||C||_F kappa_2(A) e / (sqrt(2) (1 - kappa_2(A) e)),  e = eps_dev + eps_host,
    so a column differs by at most ||eps_s||_2 times that, plus the bound above."""
import numpy as np

from oracle_context import OracleContext

U = 2.0 ** -53
FACTOR_RATIO = 4e-15


def gamma(m):
    return m * U / (1.0 - m * U)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def factor_ratio(A, C):
    """||A - C C'||_F / ||A||_F."""
    return float(np.linalg.norm(A - C @ C.T) / np.linalg.norm(A))


def check_factor(tag, A, C):
    """Check 1: lower triangular with exact zeros above, a positive diagonal, and the backward error of the factorisation."""
    assert C.shape == A.shape
    assert not np.any(np.triu(C, 1)), tag
    assert np.all(np.diag(C) > 0.0), tag
    ratio = factor_ratio(A, C)
    print(f"\n{tag}: ||A - CC'||_F / ||A||_F = {ratio:.3g}")
    assert ratio <= FACTOR_RATIO, (tag, ratio)
    return ratio


def draw_bound(C, eps, mu):
    """Entrywise bound of check 2, (nt, S)."""
    nt = C.shape[0]
    return 2.0 * gamma(nt + 2) * (np.abs(C) @ np.abs(eps) + np.abs(mu)[:, None])


def check_draws(tag, out, mu, C, eps):
    """Check 2: the draws against mu + C eps formed in float64 from the device's own factor."""
    ref = mu[:, None] + C @ eps
    bound = draw_bound(C, eps, mu)
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, 0.0))) if err.size else 0.0
    print(f"\n{tag}: max |out - (mu + C eps)| = {float(np.max(err)) if err.size else 0.0:.3g}, worst err/bound {worst:.3g}")
    assert np.all(err <= bound), (tag, worst)


def sun_column_bounds(A, C_dev, C_host, eps, mu):
    """Check 3: per column, the 2-norm bound of the difference between draws through two Cholesky factors of A.  Returns
    (bounds (S,), kappa_2(A), eps_dev, eps_host)."""
    w = np.linalg.eigvalsh(A)
    kappa = float(w[-1] / w[0])
    a2 = float(w[-1])
    e_dev = float(np.linalg.norm(A - C_dev @ C_dev.T)) / a2
    e_host = float(np.linalg.norm(A - C_host @ C_host.T)) / a2
    ke = kappa * (e_dev + e_host)
    assert ke < 1.0, (kappa, e_dev, e_host)
    dC = np.linalg.norm(C_dev) * ke / (np.sqrt(2.0) * (1.0 - ke))
    own = np.linalg.norm(draw_bound(C_dev, eps, mu), axis=0)
    return np.linalg.norm(eps, axis=0) * dC + own, kappa, e_dev, e_host


class OracleSampleContext(OracleContext):
    """OracleContext that also answers predict_cov, predict_sample and predict_cov_factor in dense NumPy, with the state rule of
    the library (only after predict_run).  It records the eps it was handed."""
    route_total = 0

    def set_test(self, Xt, route_ptr, route_idx):
        super().set_test(Xt, route_ptr, route_idx)
        self.route_total = int(np.asarray(route_ptr)[-1])
        self._predicted = False
        self._factors = None

    def predict_run(self):
        self._predicted = True
        self._factors = None
        return super().predict_run()

    def predict_cov(self, leaf, nt, with_noise=True):
        assert self._predicted
        rows = self.ridx[self.rptr[leaf]:self.rptr[leaf + 1]]
        g = self.gps[leaf]
        _, S = g.prediction(self.Xt[rows], full_cov=True)
        S = np.array(S, order="F")
        if not with_noise:
            S[np.diag_indices(rows.size)] -= g.getnoise()
        return S

    def predict_sample(self, eps, with_noise=False, jitter=None):
        assert self._predicted
        eps = np.asarray(eps, dtype=np.float64)
        assert eps.ndim == 2 and eps.shape[0] == self.route_total and eps.flags.f_contiguous
        self.last_eps = eps.copy()
        jitter = (0.0 if with_noise else 1e-8) if jitter is None else jitter
        out = np.empty(eps.shape, order="F")
        info = np.zeros(self.L, dtype=np.int32)
        self._factors = {}
        for l in range(self.L):
            a, b = int(self.rptr[l]), int(self.rptr[l + 1])
            if a == b:
                continue
            A = self.predict_cov(l, b - a, with_noise) + jitter * np.eye(b - a)
            C = np.linalg.cholesky(A)
            self._factors[l] = C
            out[a:b] = self._mu[a:b, None] + C @ eps[a:b]
        return out, info

    def predict_cov_factor(self, leaf, nt):
        assert self._factors is not None
        return np.array(self._factors[leaf], order="F")
