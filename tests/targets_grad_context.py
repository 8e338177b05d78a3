"""TargetsOracleContext (tests/targets_context.py) that also answers targets_gradients, and fits every kernel kind: kinds the
CPU oracle does not have (ArdLinear, ArdSEProduct, Matern, rational quadratic) get a float64 dense leaf
(tests/dense_gp.py).  targets_gradients is targets_grad_dense's textbook contraction per (leaf, column), weighted and added in
ascending column order.  Lets the CPU suite drive model.targets_objective / model.grad_targets / model.train(targets=...) end to
end without a GPU.  Also holds `default_path_results`, the values of the untouched default paths (train, grad_mll, grad_loo)
that tests/golden/targets_grad_parent.json records from the parent commit.  Test infrastructure only."""
import numpy as np

import targets_grad_dense as tgd
from dense_gp import DenseGP
from targets_context import TargetsOracleContext


class TargetsGradOracleContext(TargetsOracleContext):
    def fit(self):
        mll, info, sec = None, None, 0.0
        if all(self.hyper[k][0] <= 2 for k in self.kid):
            mll, info, sec = super().fit()
        else:
            self.gps = [DenseGP(*self.hyper[self.kid[i]], self.X[self.obs[i]], self.y[self.obs[i]], self.mean[i])
                        for i in range(self.L)]
            mll = np.array([g.mll() for g in self.gps])
            info = np.array([g.info for g in self.gps], dtype=np.int32)
        self._tZ = None                     # a fit makes the resident targets stale, as on the device
        return mll, info, sec

    def targets_gradients(self, stride, col_weight=None):
        from deepstructuredmixtures_amd import hipabi
        if getattr(self, "_tZ", None) is None:
            raise hipabi.DsmgpError(hipabi.E_STATE, "targets_gradients before solve_targets on the current fit")
        Q = self._tY.shape[1]
        W = np.ones((self.L, Q)) if col_weight is None else np.asarray(col_weight, dtype=np.float64).reshape(self.L, Q)
        out = np.zeros((self.L, stride))
        for i in range(self.L):
            kind, hyp = self.hyper[self.kid[i]]
            G = tgd.column_gradients(kind, hyp, self.X[self.obs[i]], self._tY[self.obs[i]], self._tmean[i])[0]
            out[i, :G.shape[1]] = tgd.weighted(G, W[i])
        self.targets_gradient_calls = getattr(self, "targets_gradient_calls", 0) + 1
        return out


# ------------------------------------------------------------------------------------- the default paths, as the parent has them

def _hex(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def default_path_results():
    """train (a DSMGP model and a single GP, three iterations each, on the oracle context), grad_mll (plain and with leaf
    weights) and grad_loo (on injected leaf values) as lists of hex floats: what must not move when `targets` is not given."""
    import deepstructuredmixtures_amd as dsm
    from oracle_context import OracleContext
    rng = np.random.default_rng(61)
    X = rng.uniform(size=(400, 2))
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(400)
    out = {}
    m = dsm.buildDSMGP(X, y, 2, 3, M=40, D=2, kernel=dsm.IsoSE(0.0, 0.0), logNoise=np.log(0.3), seed=3, ctx=OracleContext())
    _, hist = dsm.train(m, iterations=3, randinit=False)
    out["train_hist"], out["train_hyp"] = _hex(hist), _hex(dsm.getparams(m))
    dsm.updategradients(m)
    out["grad_mll"] = _hex(dsm.grad_mll(m))
    out["grad_mll_weighted"] = _hex(dsm.grad_mll(m, rng.random(m.L)))
    m.leaf_lpd = m.leaf_mll - rng.random(m.L)
    out["grad_loo"] = _hex(dsm.grad_loo(m))
    m2 = dsm.buildDSMGP(X, y, 2, 3, M=40, D=2, kernel=[dsm.IsoSE(0.0, 0.0), dsm.IsoLinear(0.0)], logNoise=np.log(0.3), seed=4,
                        ctx=OracleContext())
    dsm.fit(m2)
    dsm.updategradients(m2)
    out["grad_mll_kernel_vector"] = _hex(dsm.grad_mll(m2))
    m2.leaf_lpd = m2.leaf_mll - rng.random(m2.L)
    out["grad_loo_kernel_vector"] = _hex(dsm.grad_loo(m2))
    gp = dsm.GaussianProcess(X[:80], y[:80], kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.3), ctx=OracleContext())
    _, hist = dsm.train(gp, iterations=3, randinit=False)
    out["train_gp_hist"], out["train_gp_hyp"] = _hex(hist), _hex(dsm.getparams(gp.model))
    return out
