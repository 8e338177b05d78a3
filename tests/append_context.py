"""OracleContext (tests/oracle_context.py) that also answers append_rows / append_stats by refitting the grown table from scratch
on the CPU oracle: lets the CPU suite drive model.add_data end to end without a GPU.  It counts what is uploaded, and can be told
to fail like a device that is out of memory.  Test infrastructure only."""
import numpy as np

import deepstructuredmixtures_amd as dsm

from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd.tree import route_recursive
from oracle_context import OracleContext


class AppendOracleContext(OracleContext):
    def __init__(self):
        super().__init__()
        self.calls = []                 # names of the uploads and fits, in order
        self.nomem_next_append = False  # the next append_rows raises DSMGP_E_NOMEM, as a device without room for the new arenas

    def set_train(self, X, y):
        self.calls.append("set_train")
        super().set_train(X, y)

    def set_leaves(self, obs_ptr, obs_idx, kernel_id, mean):
        self.calls.append("set_leaves")
        super().set_leaves(obs_ptr, obs_idx, kernel_id, mean)

    def fit(self):
        self.calls.append("fit")
        return super().fit()

    def append_rows(self, X_new, y_new, add_ptr, add_idx, mean=None):
        self.calls.append("append_rows")
        if not self.gps:
            raise hipabi.DsmgpError(hipabi.E_STATE, "append_rows needs a current fit")
        if self.nomem_next_append:
            self.nomem_next_append = False
            raise hipabi.DsmgpError(hipabi.E_NOMEM, "injected: the new arenas do not fit")
        X_new = np.asarray(X_new, dtype=np.float64)
        y_new = np.asarray(y_new, dtype=np.float64)
        add_ptr, add_idx = np.asarray(add_ptr), np.asarray(add_idx)
        assert X_new.shape[1] == self.X.shape[1] and len(add_ptr) == self.L + 1
        N0 = self.X.shape[0]
        self.X = np.vstack([self.X, X_new])
        self.y = np.concatenate([self.y, y_new])
        for i in range(self.L):
            add = add_idx[add_ptr[i]:add_ptr[i + 1]]
            assert np.all(np.diff(add) > 0) and np.all((add >= 0) & (add < len(y_new)))
            self.obs[i] = np.concatenate([self.obs[i], N0 + add]).astype(np.int64)
        if mean is not None:
            self.mean = list(mean)
        self.last_add = np.diff(add_ptr)
        return OracleContext.fit(self)

    def append_stats(self):
        return dict(owners_continued=int(np.count_nonzero(self.last_add)), leaves_untouched=int(np.count_nonzero(self.last_add == 0)),
                    bytes_relocated=0, block_columns_factorised=0, owners_restarted=0, copies_dissolved=0)


def grow_by_hand(family, h, xn, yn):
    """The same tree with its lists grown by the test itself (the literal recursion, not the library's walk), fitted from scratch."""
    t = h.model if family == "gp" else h
    N0 = t.x.shape[0]
    if family == "gp":
        ptr, idx = np.array([0, len(yn)]), np.arange(len(yn))
    else:
        ptr, idx = route_recursive(t.root, xn)
    t.x = np.asfortranarray(np.vstack([t.x, xn]))
    t.y = np.concatenate([t.y, yn])
    for l, lf in enumerate(t.leaves):
        add = idx[ptr[l]:ptr[l + 1]]
        if add.size:
            lf.obs = np.concatenate([lf.obs, N0 + add])
            lf.nobs = int(lf.obs.size)
            if lf.mean.default:
                lf.mean = dsm.ConstMean(float(np.mean(t.y[lf.obs])), default=True)
    if t.D is not None:
        t.D = dsm.get_overlap(t.root, t.L)
    t._uploaded, t._schedule, t._route_cache = False, None, None
    dsm.fit(h)
    return h
