"""TargetsOracleContext (tests/targets_context.py) that also answers predict_gradients and predict_targets_gradients, from the
dense float64 helpers tests/predgrad_dense.py and tests/targets_inputgrad_dense.py with their own Cholesky: lets the CPU suite
drive model.predict_targets_gradients end to end without a GPU.  Test infrastructure only."""
import numpy as np

import predgrad_dense as pgd
import targets_inputgrad_dense as tid
from targets_context import TargetsOracleContext


class TargetsInputGradOracleContext(TargetsOracleContext):
    def _leaf(self, i):
        kind, h = self.hyper[self.kid[i]]
        return kind, h[:-1], float(h[-1]), self.X[self.obs[i]], self.Xt[self.ridx[self.rptr[i]:self.rptr[i + 1]]]

    def predict_gradients(self, want_var=True):
        dmu, dvar = [np.zeros((0, self.X.shape[1]))], [np.zeros((0, self.X.shape[1]))]
        for i in range(self.L):
            kind, lh, ln, X, Xt = self._leaf(i)
            if Xt.shape[0]:
                _, _, a, b = pgd.moments(kind, lh, ln, X, self.y[self.obs[i]], self.mean[i], Xt)
                dmu.append(a)
                dvar.append(b)
        return np.concatenate(dmu), (np.concatenate(dvar) if want_var else None)

    def predict_targets_gradients(self):
        out = [np.zeros((0, self.X.shape[1], self.targets_Q))]
        for i in range(self.L):
            kind, lh, ln, X, Xt = self._leaf(i)
            if Xt.shape[0]:
                out.append(tid.moments(kind, lh, ln, X, self._tY[self.obs[i]], self._tmean[i], Xt)[2])
        return np.concatenate(out)
