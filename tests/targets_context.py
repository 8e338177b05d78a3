"""OracleContext (tests/oracle_context.py) that also answers solve_targets / predict_targets / targets_fetch, from the float64
dense restatement tests/targets_dense.py on the oracle's factors: lets the CPU suite drive model.fit_targets /
model.predict_targets end to end without a GPU.  Test infrastructure only."""
import numpy as np

import targets_dense
from oracle import gp as ogp
from oracle_context import OracleContext


class TargetsOracleContext(OracleContext):
    targets_Q = 0

    def solve_targets(self, Y, mean=None):
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[:, None]
        mean = np.zeros((self.L, Y.shape[1])) if mean is None else np.asarray(mean, dtype=np.float64)
        self._tY, self._tmean = Y, mean
        self._tZ, mll = [], []
        for i, g in enumerate(self.gps):
            Z, m, _ = targets_dense.reference(g.L(), Y[self.obs[i]], mean[i])
            self._tZ.append(Z)
            mll.append(m)
        self.targets_Q = Y.shape[1]
        return np.stack(mll), 0.0

    def predict_targets(self):
        out = []
        for i, g in enumerate(self.gps):
            rows = self.ridx[self.rptr[i]:self.rptr[i + 1]]
            if rows.size:
                Ktn = ogp.kernelmatrix(g.kernel, self.Xt[rows], g.x, g.exact_dist)
                out.append(targets_dense.reference(g.L(), self._tY[self.obs[i]], self._tmean[i], Ktn)[2])
        return np.concatenate(out) if out else np.zeros((0, self.targets_Q))

    def targets_fetch(self, leaf):
        return self._tZ[int(leaf)]
