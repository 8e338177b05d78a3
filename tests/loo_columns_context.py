"""TargetsGradOracleContext (tests/targets_grad_context.py) that also answers loo_targets and loo_targets_gradients, from the
float64 dense restatement tests/loo_columns_dense.py: the moments per (leaf, column) and GPML eq. 5.13 as printed, column by
column, weighted and added in ascending column order.  Lets the CPU suite drive model.loo_targets / loo_targets_objective /
grad_loo_targets / train(targets=..., targets_objective="loo") end to end without a GPU.  Test infrastructure only."""
import numpy as np

import loo_columns_dense as lcd
from targets_grad_context import TargetsGradOracleContext


class LooColumnsOracleContext(TargetsGradOracleContext):
    def _resident(self, what):
        from deepstructuredmixtures_amd import hipabi
        if getattr(self, "_tZ", None) is None:
            raise hipabi.DsmgpError(hipabi.E_STATE, f"{what} before solve_targets on the current fit")
        return self._tY.shape[1]

    def _leaf(self, i):
        kind, hyp = self.hyper[self.kid[i]]
        return kind, np.asarray(hyp, dtype=np.float64), self.X[self.obs[i]], self._tY[self.obs[i]], self._tmean[i]

    def loo_targets(self):
        Q = self._resident("loo_targets")
        mu, var, lpd = [], [], np.zeros((self.L, Q))
        for i in range(self.L):
            m, v, lpd[i] = lcd.moments(*self._leaf(i))
            mu.append(m)
            var.append(v)
        return np.concatenate(mu, axis=0), np.concatenate(var), lpd

    def loo_targets_gradients(self, stride, col_weight=None):
        from deepstructuredmixtures_amd import hipabi
        Q = self._resident("loo_targets_gradients")
        W = np.ones((self.L, Q)) if col_weight is None else np.asarray(col_weight, dtype=np.float64).reshape(self.L, Q)
        if not np.all(np.isfinite(W)) or np.any(W < 0.0):
            raise hipabi.DsmgpError(hipabi.E_ARG, "loo_targets_gradients: non-finite or negative value in col_weight")
        out = np.zeros((self.L, stride))
        lpd = np.zeros((self.L, Q))
        for i in range(self.L):
            G = lcd.column_gradients_literal(*self._leaf(i))
            out[i, :G.shape[1]] = lcd.weighted(G, W[i])
            lpd[i] = lcd.moments(*self._leaf(i))[2]
        self.loo_targets_gradient_calls = getattr(self, "loo_targets_gradient_calls", 0) + 1
        return out, lpd
