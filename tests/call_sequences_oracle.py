"""The dense float64 chain the call sequences of tests/call_sequences.py are checked against: LooColumnsOracleContext
(tests/loo_columns_context.py) with the readers it lacks, and for every reader the reference value together with its tolerance.

Every leaf is fitted densely (tests/dense_gp.py), for all kernel kinds, so that a leaf that is not
positive definite is reported (info != 0) and gets NaN wherever the device gives NaN.  The readers the chain lacks come from the
dense modules: loo_columns_dense with one column for loo / loo_gradients, the kernel table of dense_kernels under the formulas
of predgrad_dense for predict_gradients, K_tt - V'V for predict_cov as tests/test_predcov_host.py restates it,
pred_tolerance.aggregate for the four families, targets_dense / targets_grad_dense for the target columns.

No tolerance is new.  `SeqOracleContext.reference(m, reader)` returns [(value, tolerance)] with the tolerance the named helper
derives, doubled because both sides are float64 (tests/targets_dense.py, last paragraph); `None` marks an exact comparison
(routes; the zero / nonzero pattern of info).  Test infrastructure only."""
import copy

import numpy as np
import scipy.linalg as sla

import call_sequences as cs
import dense_kernels as dk
import loo_columns_dense as lcd
import loo_dense as ld
import loo_grad_dense as lgd
import targets_dense as td
import targets_grad_dense as tgd
from dense_gp import DenseGP
from loo_columns_context import LooColumnsOracleContext
from oracle_context import OraclePartialContext
from pred_tolerance import ATOL, EPS, LOG2PI, RTOL, Prop, agg_tol, aggregate, alpha_tol, mll_tol, moment_tol, row_entries, score_tol


class Leaf(DenseGP):
    """A DenseGP kept by its inputs, with the ArdSE option the context's gradients() reads."""
    _cache = {}

    def __init__(self, kind, hyp, X, y, mean, ard_true=False):
        super().__init__(kind, hyp, X, y, mean)
        self.ard_true = ard_true

    def grad(self):
        return mll_gradients(self, self.y, [self.mean], self.ard_true)[0]


def mll_gradients(g, Y, mean, ard_true):
    """targets_grad_dense.column_gradients on a fitted leaf (its factor instead of a factorisation per call): G[Q, len(hyp)],
    every column's gradient row in the library's convention."""
    Y = Y[:, None] if Y.ndim == 1 else Y
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (Y.shape[1],))
    return tgd.gradients_from_factor(g.kind, g.hyp, g.x, g.F, Y, mean, ard_true)[0]


class SeqOracleContext(LooColumnsOracleContext):
    def __init__(self):
        super().__init__()
        self.opts = dict(cs.OPT_DEFAULT)
        self._agg = None
        self._tZ = None

    # ---- writers the chain lacks (no numerical meaning on the dense side)
    def set_option(self, option, value):
        name = {v: k for k, v in cs.OPT.items()}[int(option)]
        if name == "lanes" and not 0 <= int(value) <= 4:
            raise ValueError("lanes")
        self.opts[name] = int(value)

    def reserve(self, nbytes):
        pass

    def release(self):
        pass

    def set_leaves(self, obs_ptr, obs_idx, kernel_id, mean):
        super().set_leaves(obs_ptr, obs_idx, kernel_id, mean)
        self._grad_active = None            # a new leaf table resets the mask of set_gradient_leaves, as on the device

    def set_tree(self, kind, first_child, n_child, split_dim, thr, leaf_local):
        self._tree = True

    def set_test_routed(self, Xt):
        Xr, ptr, idx = cs.routed_testset(self.X.shape[1])
        assert np.array_equal(Xr, Xt)
        self.set_test(Xt, ptr, idx)
        return ptr

    def routes(self):
        return self.rptr, self.ridx

    # ---- fit and prediction, densely for every kind
    def fit(self):
        self.gps = []
        for i in range(self.L):
            kind, h = self.hyper[self.kid[i]]
            key = (id(self.X), kind, h.tobytes(), self.obs[i].tobytes(), float(self.mean[i]), bool(self.opts["ard"]))
            if key not in Leaf._cache:
                Leaf._cache[key] = Leaf(kind, h, self.X[self.obs[i]], self.y[self.obs[i]], self.mean[i], bool(self.opts["ard"]))
            self.gps.append(Leaf._cache[key])
        self._tZ = None
        return np.array([g.mll() for g in self.gps]), np.array([g.info for g in self.gps], dtype=np.int32), 0.0

    def _rows(self, i):
        return self.ridx[self.rptr[i]:self.rptr[i + 1]]

    def predict_run(self):
        mu, var, self._V = [], [], {}
        for i, g in enumerate(self.gps):
            rows = self._rows(i)
            if not rows.size:
                continue
            Ktn = dk.value(g.kind, g.hyp[:-1], self.Xt[rows], g.x)
            V = sla.solve_triangular(g.F, Ktn.T, lower=True)
            self._V[i] = (Ktn, V)
            m = g.mean + Ktn @ g.alpha
            v = dk.prior_diag(g.kind, g.hyp[:-1], self.Xt[rows]) - np.sum(V * V, axis=0) + g.noise
            mu.append(m if not g.info else np.full(rows.size, np.nan))
            var.append(v if not g.info else np.full(rows.size, np.nan))
        self._mu = np.concatenate(mu) if mu else np.zeros(0)
        self._var = np.concatenate(var) if var else np.zeros(0)
        return 0.0

    def predict_targets(self):
        out = []
        for i, g in enumerate(self.gps):
            if i in self._V:
                mu = td.reference(g.F, self._tY[self.obs[i]], self._tmean[i], self._V[i][0])[2]
                out.append(mu if not g.info else np.full(mu.shape, np.nan))
        return np.concatenate(out) if out else np.zeros((0, self.targets_Q))

    def gradients(self, stride):
        for g in self.gps:
            g.ard_true = bool(self.opts["ard"])
        return super().gradients(stride)

    def aggregate_partial(self, family, leaf_coef=None, leaf_group=None, n_groups=0, fetch=True):
        self._agg = (family, leaf_coef, leaf_group, n_groups)
        return OraclePartialContext.aggregate_partial(self, family, leaf_coef, leaf_group, n_groups)

    def _finish(self):
        family, coef, group, G = self._agg
        ent = row_entries(self.rptr, self.ridx, self.Xt.shape[0])
        g0 = self.hyper[0]
        kw = dict(coef=coef, group=group, G=G, plain=False)
        if family == 3:
            kw.update(kss_prior=dk.prior_diag(g0[0], g0[1][:-1], self.Xt), noise_prior=float(np.exp(2.0 * g0[1][-1])))
        with np.errstate(all="ignore"):
            m, v = aggregate(family, list(self._mu), list(self._var), ent, log=np.log, **kw)
        self._amu, self._avar = np.array(m, dtype=np.float64), np.array(v, dtype=np.float64)
        return self._amu, self._avar

    def aggregate(self, family, leaf_coef=None, leaf_group=None, n_groups=0, plain=False, prior_kernel_id=0, fetch=True):
        self._agg = (family, leaf_coef, leaf_group, n_groups)
        return self._finish()

    def aggregate_finish(self, partial=None, plain=False, prior_kernel_id=0, fetch=True):
        return self._finish()

    @staticmethod
    def _scores(y, mu, var):
        n = y.size
        se, ae = (y - mu) ** 2, np.abs(y - mu)
        return np.array([np.mean(se), np.std(se, ddof=1) / np.sqrt(n) if n > 1 else np.nan, np.mean(ae),
                         np.std(ae, ddof=1) / np.sqrt(n) if n > 1 else np.nan, np.mean(0.5 * (se / var + LOG2PI) + np.log(np.sqrt(var)))])

    def scores(self, y_test):
        return dict(zip(("mse", "sse", "mae", "sae", "nlpd"), self._scores(np.asarray(y_test), self._amu, self._avar)))

    # ---- every reader with its tolerance
    def _nan_failed(self, per_leaf):
        """Concatenate per-leaf blocks, NaN for the leaves whose fit failed."""
        return [np.full(np.shape(b), np.nan) if g.info else np.asarray(b, dtype=np.float64) for g, b in zip(self.gps, per_leaf)]

    def _entry_tols(self):
        """(tol mu, tol var) of every (leaf, routed row) entry: pred_tolerance.moment_tol."""
        kss, noise = [], []
        for i, g in enumerate(self.gps):
            rows = self._rows(i)
            kss.append(dk.prior_diag(g.kind, g.hyp[:-1], self.Xt[rows]) if rows.size else np.zeros(0))
            noise.append(np.full(rows.size, g.noise))
        kss, noise = np.concatenate(kss), np.concatenate(noise)
        tm, tv = moment_tol(self._mu, self._var, kss, noise, max(1.0, float(np.max(np.abs(self.y)))))
        return 2.0 * tm, 2.0 * tv

    def _agg_reference(self, m, family):
        L = self.L
        coef, group, G, _ = cs.agg_args(family, L)
        self._agg = (cs.FAMILY[family], coef, group, G)
        mu, var = self._finish()
        tm_e, tv_e = self._entry_tols()
        ent = row_entries(self.rptr, self.ridx, self.Xt.shape[0])
        kw = dict(coef=coef, group=group, G=G, plain=False)
        S1 = None
        if family == "mixture":
            S1 = np.array([sum(coef[l] * self._mu[e] ** 2 for l, e in er) for er in ent])
        if family == "rbcm":
            g0 = self.hyper[0]
            kw.update(kss_prior=dk.prior_diag(g0[0], g0[1][:-1], self.Xt), noise_prior=float(np.exp(2.0 * g0[1][-1])))
        with np.errstate(all="ignore"):
            tm, tv = agg_tol(cs.FAMILY[family], np.nan_to_num(self._mu), np.nan_to_num(self._var, nan=1.0), tm_e / 2.0, tv_e / 2.0, ent,
                             S1=S1, **kw)
        return mu, var, 2.0 * tm, 2.0 * tv

    def _partial_reference(self, family):
        """The partial sums with the entries' tolerances carried through them (pred_tolerance.Prop), plus agg_tol's 16 eps |value|
        for the device's own rounding of a few terms per row."""
        L = self.L
        coef, group, G, _ = cs.agg_args(family, L)
        part = self.aggregate_partial(cs.FAMILY[family], coef, group, G)
        tm, tv = self._entry_tols()
        leaf = np.repeat(np.arange(L), np.diff(self.rptr))
        mu, var, n_t = Prop(self._mu, tm / 2.0), Prop(self._var, tv / 2.0), self.Xt.shape[0]
        if family == "mixture":
            w = coef[leaf]
            terms = [mu * w, mu * mu * w, var * w]
            sel = [np.ones(leaf.size, dtype=bool)] * 3
        elif family == "rbcm":
            t = 1.0 / var
            terms, sel = [], []
            for k in range(G):
                terms += [t * mu, t]
                sel += [group[leaf] == k] * 2
        else:
            bt = (1.0 / var) * coef[leaf]
            terms, sel = [bt * mu, bt], [np.ones(leaf.size, dtype=bool)] * 2
        tol = np.stack([np.bincount(self.ridx[s], weights=t_.e[s], minlength=n_t) for t_, s in zip(terms, sel)])
        return part, 2.0 * (tol + 16 * EPS * np.abs(part))

    def reference(self, m, reader):
        """[(reference, tolerance)] of `reader` on the oracle's current state, aligned with the tuple call_sequences.read returns."""
        name, arg = cs.split(reader)
        L, D = self.L, self.X.shape[1]
        stride = D + 3
        gps = self.gps
        ok = [not g.info for g in gps] if gps else []
        if name == "fit":
            mll = np.array([g.mll() for g in gps])
            tol = np.array([2.0 * float(mll_tol(v, g.cond)) if not g.info else np.nan for v, g in zip(mll, gps)])
            return [(mll, tol), (np.array([g.info for g in gps], dtype=np.int64), None)]
        if name == "download_factor":
            out = []
            for l in sorted({0, L - 1}):
                g = gps[l]
                # The factor: tests/targets_dense.py derives z_tol in two halves, and the first IS the bound on the factor -- the
                # computed factor is the exact factor of K_y + E, |E| <= c n eps |K_y| (backward stability of Cholesky), so its
                # relative distance to the factor of K_y is at most cond_2(K_y) |E| / |K_y| / sqrt 2 (Sun 1991, Stewart 1993): of
                # the form c cond eps |F|, with that module's constant 64, column by column; both sides float64: doubled.
                out += [(g.F, 2.0 * td.z_tol(g.F, g.cond)), (g.alpha, np.full(g.alpha.size, 2.0 * alpha_tol(g.alpha, g.cond)))]
            return out
        if name == "predict_fetch":
            tm, tv = self._entry_tols()
            return [(self._mu, tm), (self._var, tv)]
        if name == "predict_cov":
            l = int(np.argmax(np.diff(self.rptr)))
            g, rows = gps[l], self._rows(l)
            kss = dk.prior_diag(g.kind, g.hyp[:-1], self.Xt[rows])
            V = self._V[l][1]
            S = dk.value(g.kind, g.hyp[:-1], self.Xt[rows], self.Xt[rows]) - V.T @ V + g.noise * np.eye(rows.size)
            # tests/test_predcov_gpu.py entry_tol, doubled
            return [(S, 2.0 * (RTOL * np.abs(S) + ATOL * np.maximum(1.0, np.maximum(kss[:, None], kss[None, :]) + g.noise)))]
        if name == "predict_gradients":
            dmu, dvar, tmu, tvar = [], [], [], []
            yscale = max(1.0, float(np.max(np.abs(self.y))))
            for i, g in enumerate(gps):
                rows = self._rows(i)
                if not rows.size:
                    continue
                Xr, h = self.Xt[rows], g.hyp[:-1]
                Gd = dk.d_input(g.kind, h, Xr, g.x)
                beta = sla.solve_triangular(g.F, self._V[i][1], lower=True, trans="T").T
                a = np.einsum("i,tid->td", np.nan_to_num(g.alpha), Gd)
                b = dk.prior_dx(g.kind, h, Xr) - 2.0 * np.einsum("ti,tid->td", beta, Gd)
                gs = dk.grad_scale(g.kind, h, g.x, Xr)
                vscale = np.maximum(1.0, dk.prior_diag(g.kind, h, Xr) + g.noise)[:, None]
                nan = np.nan if g.info else 0.0             # predgrad_dense.tolerances, doubled
                dmu.append(a + nan)
                dvar.append(b + nan)
                tmu.append(2.0 * (RTOL * np.abs(a) + ATOL * yscale * gs))
                tvar.append(2.0 * (RTOL * np.abs(b) + ATOL * vscale * gs))
            cat = lambda x: np.concatenate(x) if x else np.zeros((0, D))      # noqa: E731
            return [(cat(dmu), cat(tmu))] + ([(cat(dvar), cat(tvar))] if arg == "var" else [])
        if name == "aggregate":
            mu, var, tm, tv = self._agg_reference(m, arg)
            return [(mu, tm), (var, tv)]
        if name == "aggregate_partial":
            return [self._partial_reference(arg)]
        if name in ("aggregate_finish", "scores"):
            mu, var, tm, tv = self._agg_reference(m, m.agg[0])
            if name == "aggregate_finish":
                return [(mu, tm), (var, tv)]
            y = cs.y_test(self.Xt)
            return [(self._scores(y, mu, var), 2.0 * score_tol(y, mu, var, tm / 2.0, tv / 2.0))]
        if name == "gradients":
            act = getattr(self, "_grad_active", None)
            ref, tol = np.zeros((L, stride)), np.zeros((L, stride))
            for i, g in enumerate(gps):
                if act is not None and not act[i]:
                    continue
                if g.info:
                    ref[i] = tol[i] = np.nan
                    continue
                G = mll_gradients(g, g.y, [g.mean], bool(self.opts["ard"]))
                ref[i, :G.shape[1]] = G[0]
                tol[i] = 2.0 * tgd.tolerance(G, [1.0], g.cond)[0]
            return [(ref, tol)]
        if name in ("loo", "loo_gradients"):
            mu, var, lpd, tm, tv, tl = [], [], np.zeros(L), [], [], np.zeros(L)
            for i, g in enumerate(gps):
                if g.info:
                    nan = np.full(g.y.size, np.nan)
                    mu, var, tm, tv = mu + [nan], var + [nan], tm + [nan], tv + [nan]
                    lpd[i] = tl[i] = np.nan
                    continue
                a, b, c = lcd.moments(g.kind, g.hyp, g.x, g.y[:, None], [g.mean])
                t = ld.loo_tol(g.y, a[:, 0], b, np.diag(g.K), g.noise)
                mu, var, tm, tv = mu + [a[:, 0]], var + [b], tm + [2.0 * t[0]], tv + [2.0 * t[1]]
                lpd[i], tl[i] = c[0], 2.0 * t[3]
            if name == "loo":
                return [(np.concatenate(mu), np.concatenate(tm)), (np.concatenate(var), np.concatenate(tv)), (lpd, tl)]
            ref, tol = np.zeros((L, stride)), np.zeros((L, stride))
            for i, g in enumerate(gps):
                if g.info:
                    ref[i] = tol[i] = np.nan
                    continue
                Gc = lcd.column_gradients_literal(g.kind, g.hyp, g.x, g.y[:, None], [g.mean])[0]
                ref[i, :Gc.size] = Gc
                tol[i] = 2.0 * lgd.tolerance(dict(kind=g.kind, cond=g.cond, weak=False, logNoise=g.hyp[-1]), Gc)[0]
            return [(ref, tol), (lpd, tl)]
        # ---- the target columns
        if name == "solve_targets":
            Y, mean, _ = cs.targets(arg, m.train, m.leaves)
        else:
            Y, mean, W = cs.targets(m.targets, m.train, m.leaves) if m.targets else (None, None, None)
        if name == "solve_targets":
            ref, tol = np.zeros((L, Y.shape[1])), np.zeros((L, Y.shape[1]))
            for i, g in enumerate(gps):
                Z, mll, _ = td.reference(g.F, Y[self.obs[i]], mean[i])
                ref[i], tol[i] = (mll, 2.0 * td.mll_tol(Z, g.F, g.cond)) if not g.info else (np.nan, np.nan)
            return [(ref, tol)]
        if name == "targets_fetch":
            g = gps[L - 1]
            Z = td.reference(g.F, Y[self.obs[L - 1]], mean[L - 1])[0]
            return [(Z, 2.0 * td.z_tol(Z, g.cond))]
        if name == "predict_targets":
            mu, tol = [], []
            for i, g in enumerate(gps):
                if i in self._V:
                    a = td.reference(g.F, Y[self.obs[i]], mean[i], self._V[i][0])[2]
                    mu.append(a + (np.nan if g.info else 0.0))
                    tol.append(2.0 * td.mu_tol(a, Y[self.obs[i]]))
            Q = Y.shape[1]
            return [(np.concatenate(mu) if mu else np.zeros((0, Q)), np.concatenate(tol) if tol else np.zeros((0, Q)))]
        if name == "targets_gradients":
            ref, tol = np.zeros((L, stride)), np.zeros((L, stride))
            for i, g in enumerate(gps):
                if g.info:
                    ref[i] = tol[i] = np.nan
                    continue
                G = mll_gradients(g, Y[self.obs[i]], mean[i], bool(self.opts["ard"]))
                ref[i, :G.shape[1]] = tgd.weighted(G, W[i])
                tol[i] = 2.0 * tgd.tolerance(G, W[i], g.cond)[0]
            return [(ref, tol)]
        if name in ("loo_targets", "loo_targets_gradients"):
            Q = Y.shape[1]
            mu, var, tm, tv, lpd, tl = [], [], [], [], np.zeros((L, Q)), np.zeros((L, Q))
            for i, g in enumerate(gps):
                Yl = Y[self.obs[i]]
                if g.info:
                    mu, tm = mu + [np.full(Yl.shape, np.nan)], tm + [np.full(Yl.shape, np.nan)]
                    var, tv = var + [np.full(Yl.shape[0], np.nan)], tv + [np.full(Yl.shape[0], np.nan)]
                    lpd[i] = tl[i] = np.nan
                    continue
                a, b, c = lcd.moments(g.kind, g.hyp, g.x, Yl, mean[i])
                ts = [ld.loo_tol(Yl[:, q], a[:, q], b, np.diag(g.K), g.noise) for q in range(Q)]
                mu, tm = mu + [a], tm + [2.0 * np.stack([t[0] for t in ts], axis=1)]
                var, tv = var + [b], tv + [2.0 * np.min(np.stack([t[1] for t in ts]), axis=0)]
                lpd[i], tl[i] = c, [2.0 * t[3] for t in ts]
            if name == "loo_targets":
                return [(np.concatenate(mu), np.concatenate(tm)), (np.concatenate(var), np.concatenate(tv)), (lpd, tl)]
            ref, tol = np.zeros((L, stride)), np.zeros((L, stride))
            for i, g in enumerate(gps):
                if g.info:
                    ref[i] = tol[i] = np.nan
                    continue
                Yl = Y[self.obs[i]]
                Gc = lcd.column_gradients_literal(g.kind, g.hyp, g.x, Yl, mean[i])
                case = dict(kind=g.kind, hyp=g.hyp, cond=g.cond, weak=False, Y=Yl, mean=mean[i])
                ref[i, :Gc.shape[1]] = lcd.weighted(Gc, W[i])
                tol[i] = 2.0 * lcd.gradient_tolerance(case, Gc, W[i], g.K)[0]
            return [(ref, tol), (lpd, tl)]
        if name == "routes":
            return [(np.asarray(self.rptr, dtype=np.int64), None), (np.asarray(self.ridx, dtype=np.int64), None)]
        if name == "kernel_matrix":
            X = self.X
            out = []
            for k in sorted(m.hyper):
                kind, h = self.hyper[k]
                K = dk.value(kind, h[:-1], X[:130], X[130:263])
                out.append((K, np.full(K.shape, 1e-13 * max(1.0, float(np.max(np.abs(K)))))))     # tests/test_gpu_parity.py
            return out
        raise KeyError(reader)

    def healthy_cond(self):
        """cond_2(K_y) of every healthy leaf of the last fit."""
        return [g.cond for g in self.gps if not g.info]


STATEFUL = ("fit", "solve_targets", "aggregate", "aggregate_partial", "aggregate_finish")   # readers that also write state


class Harness:
    """Walks sequences on a SeqOracleContext kept in step with the model; reference values are memoised by the reader's inputs."""

    def __init__(self):
        self.memo = {}

    def start(self):
        self.oracle, self.m = SeqOracleContext(), cs.Model()

    def step(self, op, arg):
        """Advance model and oracle by one op.  Returns (expected code or None, the reader call or None, [(ref, tol)] or None,
        the model before the op)."""
        before = copy.deepcopy(self.m)
        code = self.m.apply(op, arg)
        call = cs.call_id(op, arg)
        if code is not None:
            return code, call, None, before
        if call is None:
            cs.run_op(self.oracle, before, op, arg)
            return None, None, None, before
        if op in STATEFUL:
            cs.read(self.oracle, before, call)
        key = before.input_key(call)
        if key not in self.memo:
            self.memo[key] = self.oracle.reference(before, call)
        return None, call, self.memo[key], before
