"""CPU tests of the host side of the full predictive covariance: model.prediction(full_cov=True), model.leaf_covariance,
model.posterior_sample and the refusals, driven through a subclass of the oracle-backed test double whose predict_cov is
oracle.gp's prediction(full_cov=True) -- "the reference as written" (src/gaussianprocess.jl:110-137)."""
import types

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi, datagen
from deepstructuredmixtures_amd.model import EPS
from deepstructuredmixtures_amd.tree import route_recursive
from oracle_context import OracleContext


class OracleCovContext(OracleContext):
    """OracleContext that also answers predict_cov, with the state rule of the library: only after predict_run."""

    def set_test(self, Xt, route_ptr, route_idx):
        super().set_test(Xt, route_ptr, route_idx)
        self._predicted = False

    def predict_run(self):
        self._predicted = True
        return super().predict_run()

    def predict_cov(self, leaf, nt, with_noise=True):
        if not getattr(self, "_predicted", False):
            raise hipabi.DsmgpError(hipabi.E_STATE, "predict_cov before predict_run")
        rows = self.ridx[self.rptr[leaf]:self.rptr[leaf + 1]]
        if nt < rows.size:
            raise hipabi.DsmgpError(hipabi.E_ARG, "ld < nt")
        g = self.gps[leaf]
        _, S = g.prediction(self.Xt[rows], full_cov=True)
        S = np.array(S, order="F")
        if not with_noise:
            S[np.diag_indices(rows.size)] -= g.getnoise()
        return S


def _problem(N=160, D=2, seed=31):
    X = datagen.uniform(seed, 0, N * D).reshape((N, D), order="F")
    y = np.sin(5 * X[:, 0]) + 0.5 * X[:, -1] + 0.1 * datagen.normal(seed + 1, 0, N)
    Xt = datagen.uniform(seed + 2, 0, 30 * D).reshape((30, D), order="F")
    return X, y, Xt


def _gp(X, y):
    return dsm.GaussianProcess(X, y, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), ctx=OracleCovContext(),
                               run_cholesky=True)


def test_prediction_full_cov_returns_the_reference_matrix():
    X, y, Xt = _problem()
    gp = _gp(X, y)
    mu0, var0 = dsm.prediction(gp, Xt)
    mu, S = dsm.prediction(gp, Xt, full_cov=True)
    mo, So = gp.model.ctx.gps[0].prediction(Xt, full_cov=True)
    assert S.shape == (30, 30) and np.array_equal(S, So) and np.array_equal(mu, mo)
    assert np.array_equal(mu, mu0)
    assert np.allclose(np.diag(S), var0, rtol=1e-10, atol=1e-12)
    mu1, var1 = dsm.prediction(gp, Xt, full_cov=False)                       # the default is untouched
    assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0) and var1.shape == (30,)
    e_mu, e_S = dsm.prediction(gp, np.zeros((0, 2)), full_cov=True)
    assert e_mu.shape == (0,) and e_S.shape == (0, 0)
    with pytest.raises(ValueError):                                          # wrong width
        dsm.prediction(gp, np.zeros((4, 3)), full_cov=True)


def test_leaf_covariance_rows_and_matrix_against_a_hand_routed_oracle():
    X, y, Xt = _problem(N=400)
    m = dsm.buildDSMGP(X, y, 2, 3, M=40, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), seed=5, ctx=OracleCovContext())
    hptr, hidx = route_recursive(m.root, Xt)       # the reference's recursion, one node at a time
    seen = 0
    for leaf in range(m.L):
        rows, S = dsm.leaf_covariance(m, Xt, leaf, with_noise=False)
        want = hidx[hptr[leaf]:hptr[leaf + 1]]
        assert np.array_equal(rows, want)
        if rows.size == 0:
            assert S.shape == (0, 0)
            continue
        seen += 1
        g = m.ctx.gps[leaf]
        _, So = g.prediction(Xt[rows], full_cov=True)
        So[np.diag_indices(rows.size)] -= g.getnoise()
        assert np.array_equal(S, So)
        _, Sn = dsm.leaf_covariance(m, Xt, leaf)                            # noise on the diagonal by default
        assert np.allclose(np.diag(Sn) - np.diag(S), g.getnoise(), rtol=1e-9) and np.array_equal(Sn - np.diag(np.diag(Sn)), S - np.diag(np.diag(S)))
    assert seen >= 2
    with pytest.raises(ValueError):
        dsm.leaf_covariance(m, Xt, m.L)
    with pytest.raises(ValueError):
        dsm.leaf_covariance(m, np.zeros((4, 3)), 0)


def test_posterior_sample_shape_determinism_and_arithmetic():
    X, y, Xt = _problem()
    gp = _gp(X, y)
    nt, ns = Xt.shape[0], 7
    s = dsm.posterior_sample(gp, Xt, ns, seed=11)
    assert s.shape == (ns, nt)
    assert np.array_equal(s, dsm.posterior_sample(gp, Xt, ns, seed=11))
    assert not np.array_equal(s, dsm.posterior_sample(gp, Xt, ns, seed=12))
    mu, Sn = dsm.prediction(gp, Xt, full_cov=True)
    S0 = gp.model.ctx.predict_cov(0, nt, with_noise=False)
    eps = datagen.normal(11, 0, nt * ns).reshape((nt, ns), order="F")
    # mu + chol(Sigma + EPS I) eps, operation for operation (samples - mu itself rounds once more)
    Lc = np.linalg.cholesky(S0 + EPS * np.eye(nt))
    assert np.array_equal(s, (mu[:, None] + Lc @ eps).T)
    assert np.allclose(s - mu[None, :], (Lc @ eps).T, rtol=0, atol=1e-13)
    sn = dsm.posterior_sample(gp, Xt, ns, seed=11, with_noise=True)        # the noisy law: no EPS
    assert np.array_equal(sn, (mu[:, None] + np.linalg.cholesky(Sn) @ eps).T)
    assert dsm.posterior_sample(gp, Xt, 0).shape == (0, nt)
    assert dsm.posterior_sample(gp, np.zeros((0, 2)), 3).shape == (3, 0)


def test_posterior_sample_raises_when_the_cholesky_fails():
    X, y, Xt = _problem()
    gp = _gp(X, y)

    def indefinite(leaf, nt, with_noise=True):
        S = np.zeros((nt, nt), order="F")
        S[0, 0] = -1.0
        return S

    gp.model.ctx.predict_cov = indefinite
    with pytest.raises(np.linalg.LinAlgError):
        dsm.posterior_sample(gp, Xt, 2)


def test_refusals():
    X, y, Xt = _problem(N=400)
    m = dsm.buildDSMGP(X, y, 2, 3, M=40, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), seed=5, ctx=OracleCovContext())
    with pytest.raises(TypeError):
        dsm.posterior_sample(m, Xt, 2)                                      # a mixture has no joint Gaussian law
    # two ranks, this one holds leaves 0 and 1: any other leaf is refused before anything is sent anywhere
    m.shard = types.SimpleNamespace(world=2, local=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        dsm.leaf_covariance(m, Xt, m.L - 1)
    # the contexts that cannot serve it say so
    for cls in (hipabi.MultiContext, hipabi.StreamingContext):
        obj = cls.__new__(cls)                                              # no device: the refusal needs no state
        with pytest.raises(hipabi.DsmgpError, match="predict_cov"):
            obj.predict_cov(0, 4)
    assert "dsmgp_predict_cov" in hipabi.SIGNATURES
