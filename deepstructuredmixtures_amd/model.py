"""Host-side mirror of the reference's model API over the HIP GP-expert path.

Names and argument meaning follow the Julia package (`!` dropped): buildDSMGP / buildPoE / buildBCM
(`src/treeStructure.jl:328-403`), fit / fit_naive (`src/fit.jl:67-122,294-304`), predict
(`src/common.jl:294-307`), update / infer / mll (`src/common.jl:323-355`, `src/optimize.jl:18-25`),
setparams / getparams (`src/optimize.jl:185-198`), train (`src/optimisers.jl:4-87`).

All per-leaf numerics (Gram, Cholesky, alpha, mll, predictive moments, gradients) are computed by
libdsmgp_hip.so through `hipabi.Context`; this module only holds the tree logic the reference keeps in
scalar Julia code (routing, log-domain mixture aggregation, weights), plus leaf sharding across ranks.
"""
import inspect

import numpy as np

try:
    import xxhash as _xxhash
except ImportError:          # pragma: no cover
    _xxhash = None

from . import hipabi
from .kernels import (IsoSE, ConstMean, KIND_ISO_SE, KIND_ARD_SE, KIND_ISO_LINEAR, KIND_ARD_LINEAR, KIND_ARD_SE_PRODUCT,
                      KIND_ISO_MATERN32, KIND_ISO_MATERN52, KIND_ARD_MATERN32, KIND_ARD_MATERN52, KIND_ISO_RQ, KIND_ARD_RQ)
from .tree import (DSMGPConfig, GPSumNode, build_tree, get_leaves, get_overlap, obs_table, share_schedule, share_decisions,
                   share_census, route, route_all, route_index, get_child, ordered_nodes, SHARE_COPY, SHARE_FULL, SHARE_PREFIX)
from . import dist as _dist
from . import datagen as _datagen

EPS = 1e-8  # `const ϵ` of src/DeepStructuredMixtures.jl:27


def _logsumexp(a, axis=None):
    """StatsFuns.logsumexp / `lse` (`src/common.jl:309-313`): max-shifted."""
    a = np.asarray(a, dtype=np.float64)
    if axis is None:
        m = np.max(a)
        m = m if np.isfinite(m) else 0.0
        return float(np.log(np.sum(np.exp(a - m))) + m)
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return np.squeeze(np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True)) + m, axis=axis)


class TreeIndex:
    """Level-order index of the sum/split tree so that the bottom-up passes of `update!`/`infer!`/`mll`
    (`src/common.jl:323-355`, `src/optimize.jl:18-25`) and the top-down product of sum-node weights on a leaf's path
    run as one vector operation per tree level instead of a Python recursion per node (18k leaves at depth 4).
    Every sum node's `logweights` becomes a view into one flat edge array, so in-place updates are seen by the
    literal recursions too."""

    def __init__(self, root):
        nodes, depth, parent_edge = [root], [0], [-1]
        levels = []            # per depth d: internal nodes at d and their child edges (children sit at d + 1)
        frontier = [0]
        edge_child, edge_parent = [], []
        d = 0
        while frontier:
            par, seg, cnt, nxt = [], [], [], []
            e0 = len(edge_child)
            for ni in frontier:
                nd = nodes[ni]
                if nd.kind == "gp":
                    continue
                par.append(ni)
                seg.append(len(edge_child) - e0)
                cnt.append(len(nd.children))
                for c in nd.children:
                    nodes.append(c)
                    depth.append(d + 1)
                    parent_edge.append(len(edge_child))
                    edge_child.append(len(nodes) - 1)
                    edge_parent.append(ni)
                    nxt.append(len(nodes) - 1)
            if par:
                levels.append(dict(parent=np.array(par), seg=np.array(seg), cnt=np.array(cnt), e0=e0,
                                   e1=len(edge_child)))
            frontier = nxt
            d += 1
        self.nodes = nodes
        self.n = len(nodes)
        self.edge_child = np.array(edge_child, dtype=np.int64)
        self.edge_parent = np.array(edge_parent, dtype=np.int64)
        self.parent_edge = np.array(parent_edge, dtype=np.int64)
        is_sum = np.array([nd.kind == "sum" for nd in nodes])
        of_gps = np.array([nd.kind == "sum" and nd.of_gps for nd in nodes])
        nch = np.array([0 if nd.kind == "gp" else len(nd.children) for nd in nodes], dtype=np.float64)
        self.edge_is_sum = is_sum[self.edge_parent] if self.edge_parent.size else np.zeros(0, bool)
        self.edge_of_gps = of_gps[self.edge_parent] if self.edge_parent.size else np.zeros(0, bool)
        self.edge_prior = np.where(self.edge_is_sum, -np.log(np.maximum(nch[self.edge_parent], 1.0)), 0.0) \
            if self.edge_parent.size else np.zeros(0)
        self.leaf_node = np.array([i for i, nd in enumerate(nodes) if nd.kind == "gp"], dtype=np.int64)
        self.leaf_id = np.array([nodes[i].leaf for i in self.leaf_node], dtype=np.int64)
        for lv in levels:
            lv["parent_is_sum"] = is_sum[lv["parent"]]
        self.levels = levels
        self.lw = np.zeros(self.edge_child.size)       # log weight per edge (0 under split nodes)
        self.bind()

    def bind(self):
        """(Re)attach every sum node's logweights to the flat edge array, keeping the current values."""
        for lv in self.levels:
            for ni, a, k in zip(lv["parent"], lv["seg"] + lv["e0"], lv["cnt"]):
                nd = self.nodes[ni]
                if nd.kind == "sum":
                    self.lw[a:a + k] = nd._lw
                    nd._lw = self.lw[a:a + k]
        self.version = GPSumNode.assignments

    def bound(self):
        return self.version == GPSumNode.assignments

    def bottom_up(self, leaf_values, posterior="all"):
        """Node values of the mll recursion; posterior: "all" = update!, "gps" = infer!, None = leave weights."""
        val = np.empty(self.n)
        val[self.leaf_node] = leaf_values[self.leaf_id]
        for lv in reversed(self.levels):
            sl = slice(lv["e0"], lv["e1"])
            v = val[self.edge_child[sl]] + self.edge_prior[sl]
            m = np.maximum.reduceat(v, lv["seg"])
            m = np.where(np.isfinite(m), m, 0.0)
            z = m + np.log(np.add.reduceat(np.exp(v - np.repeat(m, lv["cnt"])), lv["seg"]))
            tot = np.add.reduceat(v, lv["seg"])
            val[lv["parent"]] = np.where(lv["parent_is_sum"], z, tot)
            if posterior is not None:
                post = v - np.repeat(z, lv["cnt"])
                if posterior == "gps":
                    post = np.where(self.edge_of_gps[sl], post, self.edge_prior[sl])
                self.lw[sl] = np.where(self.edge_is_sum[sl], post, 0.0)
        return val

    def weights_normalised(self, tol=1e-12):
        """Do the weights of every sum node add up to one?  Every path of the reference keeps them so (-log V at build,
        `src/treeStructure.jl:226`; log Dirichlet draws, `:260-286`; the posterior of `update!` / `infer!`,
        `src/common.jl:326-353`) -- but `logweights` is a plain field a caller may assign."""
        if not self.lw.size or not np.any(self.edge_is_sum):
            return True
        tot = np.bincount(self.edge_parent[self.edge_is_sum], weights=np.exp(self.lw[self.edge_is_sum]), minlength=self.n)
        par = np.unique(self.edge_parent[self.edge_is_sum])
        return bool(np.all(np.abs(tot[par] - 1.0) <= tol))

    def leaf_path_logweights(self):
        """log of the product of sum-node weights on every leaf's path, indexed by leaf id."""
        acc = np.zeros(self.n)
        for lv in self.levels:
            sl = slice(lv["e0"], lv["e1"])
            acc[self.edge_child[sl]] = acc[self.edge_parent[sl]] + self.lw[sl]
        out = np.zeros(self.leaf_id.size)
        out[self.leaf_id] = acc[self.leaf_node]
        return out


class Model:
    """Common state of DSMGP / PoE / gPoE / rBCM (`src/DeepStructuredMixtures.jl:108-130`)."""
    family = "dsmgp"

    def __init__(self, root, x, y, overlap, ctx=None, device=0, shard=None, n_sub=1, stream_budget=None):
        self.root = root
        self.x = np.asfortranarray(x, dtype=np.float64)
        self.y = np.ascontiguousarray(y, dtype=np.float64)
        self.D = overlap  # leaf-overlap matrix (the reference calls this field D)
        self.leaves = get_leaves(root)
        self.L = len(self.leaves)
        self.shard = shard if shard is not None else _dist.Shard.single(self.L)
        self._ctx = ctx
        self._device = device
        self._n_sub = int(n_sub)      # > 1: that many concurrent contexts on this GPU (hipabi.MultiContext)
        self._stream_budget = stream_budget   # bytes (or "auto"): factor-and-discard over leaf groups (hipabi.StreamingContext)
        self.leaf_mll = np.full(self.L, np.nan)
        self.leaf_info = np.zeros(self.L, dtype=np.int32)
        self.last_fit_seconds = 0.0
        self.last_predict_seconds = 0.0
        self._uploaded = False
        self._schedule = None
        self._route_cache = None
        self._device_routing = False  # the context holds the tree (dsmgp_set_tree): predict routes its rows on the device
        self._tindex = None
        self.share_op = None          # per leaf: what the last fit did (SHARE_FULL / COPY / PREFIX)
        self.share_branch = None      # per leaf: the arm of the reference's fit! (tree.BRANCH_*)
        self.fit_census = None        # tree.share_census(share_branch): counts + the leaves of the arms computed in full here

    @property
    def tindex(self):
        if self._tindex is None:
            self._tindex = TreeIndex(self.root)
        elif not self._tindex.bound():      # somebody assigned fresh logweights arrays: take them over
            self._tindex.bind()
        return self._tindex

    @property
    def ctx(self):
        """GPU context, created on first use; raises if the HIP library or a GPU is missing."""
        if self._ctx is None:
            if self._stream_budget is not None:
                b = None if self._stream_budget == "auto" else int(self._stream_budget)
                self._ctx = hipabi.StreamingContext(self._device, b)
            elif self._n_sub > 1:
                self._ctx = hipabi.MultiContext(self._device, self._n_sub)
            else:
                self._ctx = hipabi.Context(self._device)
                if self.shard.world > 1:      # opt-in (DSMGP_EXCHANGE=rccl-device): the exchanges run through the library's
                    self.shard.device_comm(self._ctx)     # communicator; a collective every rank enters, or none
        return self._ctx

    # ---- kernel ids -> shared hyper-parameters --------------------------------------------------
    def kernel_table(self):
        """One (kernel, logNoise) per kernel id, taken from the first leaf carrying that id: the
        reference sets every leaf of an id to the same vector (`src/optimize.jl:188-198`)."""
        if getattr(self, "_ktab", None) is None:      # which leaf carries an id first is structural: cache it
            tab = {}
            for lf in self.leaves:
                tab.setdefault(lf.kernelid, lf)
            self._ktab = [tab[k] for k in sorted(tab)]
        return self._ktab

    def _push_hyper(self):
        for lf in self.kernel_table():
            hyp = np.concatenate([lf.kernel.loghyp(), [lf.logNoise]])
            self.ctx.set_hyper(lf.kernelid, lf.kernel.kind, hyp)

    def set_option(self, option, value):
        """`dsmgp_set_option` on the model's context.  An option that rebuilds the plan (OPT_FUSED_GRAM) drops the
        device-side test set with it: the route cache is told, so the next predict registers its rows again."""
        self.ctx.set_option(option, value)
        if self._route_cache is not None:
            self._route_cache["uploaded"] = False

    def _set_decisions(self, dec):
        """Record the sharing decisions of this fit (None: fit_naive!, every leaf in full) for the caller: which leaves
        the reference's default fit! would have sent through its (defective) row-deletion arm is part of the
        result, not only of the oracle."""
        if dec is None:
            dec = (np.zeros(self.L, dtype=np.int32), np.full(self.L, -1, dtype=np.int32), np.zeros(self.L, dtype=np.int64),
                   np.zeros(self.L, dtype=np.int8))
        self.share_op, self.share_branch = dec[0], dec[3]
        self.fit_census = share_census(dec[3])
        return dec

    # ---- leaf table ------------------------------------------------------------------------------
    def _upload(self, tau):
        loc = self.shard.local
        key = ("sched", None if tau is None else float(tau))
        if self._uploaded and self._schedule == key:
            return
        if len(loc) == 0:
            # a rank without leaves (fewer sharing groups than ranks, e.g. a small PoE on 8 GPUs) makes no device
            # call at all; it still joins every collective with empty contributions (_fit, _leaf_moments, ...)
            self._uploaded = True
            self._schedule = key
            self._route_cache = None
            if self.D is not None and tau is not None:
                self._set_decisions(share_decisions(self.leaves, self.D, tau))
            else:
                self._set_decisions(None)
            return
        if not self._uploaded:
            self.ctx.set_train(self.x, self.y)
        lv = [self.leaves[i] for i in loc]
        ptr, idx = obs_table(lv)
        self.ctx.set_leaves(ptr, idx, [lf.kernelid for lf in lv], [lf.mean.m for lf in lv])
        if self.D is not None and tau is not None:
            op, src, plen, _ = self._set_decisions(share_decisions(self.leaves, self.D, tau))
            self.ctx.set_sharing(*self.shard.subset.take_sharing(op, src, plen))   # (a source must live on the same rank)
        else:
            self._set_decisions(None)
            self.ctx.set_sharing(None, None, None)
        self._uploaded = True
        self._schedule = key
        self._route_cache = None      # set_leaves dropped the device-side test set
        self._register_tree()

    def _register_tree(self):
        """The routing of `predict` (`src/common.jl:101-122,181-196,275-292`) on the device: hand the context the tree as flat
        arrays, with every region's index in THIS rank's leaf table (-1: held elsewhere).  DSMGP models on a plain context;
        anything else (and a tree deeper than the device walk's stack) keeps routing on the host."""
        self._device_routing = False
        if self.family != "dsmgp" or self.root.kind == "gp" or not hasattr(self.ctx, "set_tree"):
            return
        ri = route_index(self.root)
        leaf_local = np.where(ri.leaf >= 0, self.shard.subset.global_to_local()[np.maximum(ri.leaf, 0)], -1)
        try:
            self.ctx.set_tree(ri.kind, ri.first, ri.nchild, ri.sdim, ri.thr, leaf_local)
            self._device_routing = True
        except hipabi.DsmgpError:
            pass


class DSMGP(Model):
    family = "dsmgp"


class PoE(Model):
    family = "poe"


class gPoE(Model):
    family = "gpoe"


class rBCM(Model):
    family = "rbcm"


# ------------------------------------------------------------------------------------ builders

def build(x, y, K, V, eps, M, D, kernel, meanFun, logNoise, useSum, *, seed=7, device=0, ctx=None,
          cls=DSMGP, tau=0.05, fit_now=True, shard_world=None, n_sub=1, stream_budget=None):
    """`src/treeStructure.jl:405-437`. NOTE the reference swaps its positional K/V into the config:
    config.K (splits per split node) = V argument, config.V (children per sum node) = K argument."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(-1, 1)
    config = DSMGPConfig(meanFun, kernel, logNoise, M, V, K, D, eps, useSum)
    root = build_tree(x, np.asarray(y, dtype=np.float64), config, seed=seed)
    L = len(get_leaves(root))
    overlap = get_overlap(root, L)
    model = cls(root, x, y, overlap, ctx=ctx, device=device, n_sub=n_sub, stream_budget=stream_budget)
    if shard_world is not None:
        rank, world = shard_world
        op, src, _ = share_schedule(model.leaves, overlap, tau)
        model.shard = _dist.Shard.lpt([lf.nobs for lf in model.leaves], op, src, rank, world)
    if fit_now:
        fit(model, tau=tau)
    return model


def buildDSMGP(x, y, K, V, *, eps=0.5, M=30, D=2, kernel=None, meanFun=None, logNoise=1.0, sum=True, **kw):
    """buildDSMGP(x, y, K, V): K children under each sum node, V splits per split node
    (`src/treeStructure.jl:309-339`; README.md:51 calls it as buildDSMGP(x, y, 3, 4))."""
    kernel = IsoSE(1.0, 1.0) if kernel is None else kernel
    return build(x, y, K, V, eps, M, D, kernel, meanFun, logNoise, sum, cls=DSMGP, **kw)


def buildPoE(x, y, V, *, eps=0.0, M=30, D=2, kernel=None, meanFun, logNoise=1.0, generalized=False, **kw):
    """`src/treeStructure.jl:341-371` (meanFun is a required keyword there too)."""
    kernel = IsoSE(1.0, 1.0) if kernel is None else kernel
    return build(x, y, 1, V, eps, M, D, kernel, meanFun, logNoise, False, cls=gPoE if generalized else PoE, **kw)


def buildBCM(x, y, V, *, eps=0.0, M=30, D=2, kernel=None, meanFun=None, logNoise=1.0, robust=False, **kw):
    """`src/treeStructure.jl:373-403`: always the robust BCM."""
    kernel = IsoSE(1.0, 1.0) if kernel is None else kernel
    return build(x, y, 1, V, eps, M, D, kernel, meanFun, logNoise, False, cls=rBCM, **kw)


class GaussianProcess:
    """Single exact GP (`src/gaussianprocess.jl:14-80`) as a one-leaf table on the device."""

    def __init__(self, x, y, *, mean=None, kernel=None, logNoise=np.log(7.0), run_cholesky=False, device=0, ctx=None):
        from .tree import GPNode
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        y = np.asarray(y, dtype=np.float64)
        mean = ConstMean(float(np.mean(y)), default=True) if mean is None else mean
        kernel = IsoSE(0.0, 0.0) if kernel is None else kernel
        N, D = x.shape
        leaf = GPNode(np.arange(N), np.full(D, -np.inf), np.full(D, np.inf), kernel, 0, mean, logNoise)
        leaf.leaf = 0
        self.node = leaf
        self.model = Model(leaf, x, y, None, ctx=ctx, device=device)
        self.N, self.D = N, D
        if run_cholesky:
            update_cholesky(self)

    @property
    def kernel(self):
        return self.node.kernel

    @property
    def logNoise(self):
        return self.node.logNoise


def update_cholesky(gp):
    """`update_cholesky!(gp)` (`src/gaussianprocess.jl:82-108`)."""
    fit_naive(gp.model)
    return gp


def prediction(gp, xtest, full_cov=False, input_gradients=False):
    """`prediction(gp, xtest)` -> (mu, diag of Sigma) (`src/gaussianprocess.jl:110-137`; only the
    diagonal of Sigma is ever consumed, `src/common.jl:136,147`).  `full_cov=True` -> (mu, Sigma) as the reference returns
    them: the full n_t x n_t matrix K_tt - V'V + noise I from the device (`Context.predict_cov`), symmetric to the bit.
    `input_gradients=True` -> (mu, var, dmu, dvar) with the (n_t, D) gradients of both moments with respect to the test
    point, from the device (`Context.predict_gradients`; no reference counterpart)."""
    xt = _test_matrix(gp.model, xtest)
    if input_gradients and full_cov:
        raise ValueError("prediction: full_cov and input_gradients are separate calls")
    if xt.shape[0] == 0:
        if input_gradients:
            return np.zeros(0), np.zeros(0), np.zeros((0, xt.shape[1])), np.zeros((0, xt.shape[1]))
        return np.zeros(0), (np.zeros((0, 0)) if full_cov else np.zeros(0))
    # registered like the test set of a tree model (cached by content): a loop of update_cholesky! + prediction on the same
    # rows carries them through the factorisation launches from its second pass on, and prediction only finishes the moments
    rc = _routing(gp.model, xt)
    mu, var = _leaf_moments(gp.model, xt, rc)
    if full_cov:
        return mu, gp.model.ctx.predict_cov(0, xt.shape[0], True)
    if input_gradients:
        dmu, dvar = gp.model.ctx.predict_gradients()
        return mu, var, dmu, dvar
    return mu, var


def leaf_covariance(model, xtest, leaf, with_noise=True):
    """(rows, Sigma) of one leaf of a tree model: the rows of `xtest` routed to leaf `leaf` (ascending) and their joint
    predictive covariance under that leaf's GP, K_tt - V'V (+ noise I), from the device.  Leaf level only: the joint law of
    a mixture over several leaves is not Gaussian and is not what the reference computes.  Single rank, or the owning rank of
    the leaf: with `shard.world > 1` a leaf another rank holds raises NotImplementedError."""
    if isinstance(model, GaussianProcess):
        model = model.model
    leaf = int(leaf)
    if not 0 <= leaf < model.L:
        raise ValueError(f"leaf {leaf}: the model has {model.L} leaves")
    if model.shard.world > 1 and leaf not in model.shard.local:
        raise NotImplementedError(f"leaf {leaf} is held by another rank: leaf_covariance serves this rank's leaves only")
    xt = _test_matrix(model, xtest)
    rc = _routing(model, xt)
    rows = np.asarray(rc["idx"][rc["ptr"][leaf]:rc["ptr"][leaf + 1]], dtype=np.int64)
    if rows.size == 0:
        return rows, np.zeros((0, 0))
    if not rc["uploaded"]:
        model.ctx.set_test(xt, rc["lptr"], rc["lidx"])      # (host lists: the rows come back in THIS order)
        rc["uploaded"] = True
    model.last_predict_seconds = model.ctx.predict_run()
    return rows, model.ctx.predict_cov(int(model.shard.subset.global_to_local()[leaf]), rows.size, with_noise)


def posterior_sample(gp, xtest, n_samples, seed=0, with_noise=False, device=False):
    """`n_samples` joint draws of a GaussianProcess at the rows of `xtest`: mu + chol(Sigma) eps, an (n_samples, n_t) array.
    Sigma comes from the device (`Context.predict_cov`), the factorisation and the draws run on the host; eps is the
    project's counter stream (`datagen.normal(seed, 0, n_t * n_samples)`, one column of n_t per sample).  Without noise the
    module's EPS is added to the diagonal; np.linalg.LinAlgError if the Cholesky still fails.
    `device=True`: the same eps through `Context.predict_sample` -- Sigma, its factorisation and the product stay on the device,
    nothing of size n_t^2 is downloaded; the same law, the bits of another Cholesky."""
    if not isinstance(gp, GaussianProcess):
        raise TypeError("posterior_sample takes a GaussianProcess (the joint law of a mixture is not Gaussian)")
    n_samples = int(n_samples)
    if n_samples < 0:
        raise ValueError("n_samples must not be negative")
    mu, _ = prediction(gp, xtest)
    nt = mu.size
    if nt == 0:
        return np.zeros((n_samples, 0))
    if device:
        if n_samples == 0:
            return np.zeros((0, nt))
        eps = _datagen.normal(int(seed), 0, nt * n_samples).reshape((nt, n_samples), order="F")
        draws, info = gp.model.ctx.predict_sample(eps, with_noise=with_noise)
        if info[0] != 0:
            raise np.linalg.LinAlgError(f"posterior_sample: the covariance is not positive definite (info = {int(info[0])})")
        return draws.T
    S = gp.model.ctx.predict_cov(0, nt, with_noise)
    if not with_noise:
        d = np.arange(nt)
        S[d, d] += EPS
    Lc = np.linalg.cholesky(S)
    eps = _datagen.normal(int(seed), 0, nt * n_samples).reshape((nt, n_samples), order="F")
    return (mu[:, None] + Lc @ eps).T


def leaf_samples(model, xtest, n_samples, seed=0, with_noise=False):
    """Joint draws of EVERY leaf GP at its routed rows, on the device (`Context.predict_sample`): returns
    `(route_ptr, route_idx, draws, info)` -- the routes of `xtest` as CSR over the leaves, draws `(route_total, n_samples)` in
    entry order (column s is one joint draw of every leaf; leaves are independent of each other) and the per-leaf info of the
    factorisations (a leaf with info != 0 has NaN entries).  eps = `datagen.normal(seed, 0, route_total * n_samples)` in entry
    order, one column per draw.  Without noise the module's EPS is added to the diagonals.  For DSMGP, PoE, gPoE, rBCM models
    and a GaussianProcess; single rank (`shard.world > 1` raises NotImplementedError, as `leaf_covariance` does for a leaf held
    elsewhere).  Draws of the target columns of `fit_targets` differ from these by the mean only and are not offered."""
    if isinstance(model, GaussianProcess):
        model = model.model
    n_samples = int(n_samples)
    if n_samples < 0:
        raise ValueError("n_samples must not be negative")
    if model.shard.world > 1:
        raise NotImplementedError("leaf_samples runs on a single rank")
    xt = _test_matrix(model, xtest)
    rc = _routing(model, xt)
    ptr, idx = rc["ptr"], rc["idx"]
    total = int(ptr[-1])
    if total == 0 or n_samples == 0:
        return ptr, idx, np.zeros((total, n_samples), order="F"), np.zeros(model.L, dtype=np.int32)
    if not rc["uploaded"]:
        model.ctx.set_test(xt, rc["lptr"], rc["lidx"])      # (host lists: the entries come back in THIS order)
        rc["uploaded"] = True
    model.last_predict_seconds = model.ctx.predict_run()
    eps = _datagen.normal(int(seed), 0, total * n_samples).reshape((total, n_samples), order="F")
    draws, info = model.ctx.predict_sample(eps, with_noise=with_noise)
    return ptr, idx, draws, info


_SELECTION_SEED_XOR = 0x5DEECE66D


def _sum_nodes(root):
    """The sum nodes of a tree in creation order (the counter of their ids)."""
    out, stack = [], [root]
    while stack:
        nd = stack.pop()
        if nd.kind == "sum":
            out.append(nd)
        stack.extend(nd.children)
    return sorted(out, key=lambda nd: int(nd.id.split("#")[1]))


def _mixture_choices(root, n_samples, seed):
    """(n_samples, number of sum nodes) child indices: per draw, one child of every sum node (creation order) with probability
    exp(logweights) normalised, from `datagen.Stream((seed XOR 0x5DEECE66D) mod 2^63)` -- draw after draw, node after node, one
    uniform each."""
    nodes = _sum_nodes(root)
    stream = _datagen.Stream((int(seed) ^ _SELECTION_SEED_XOR) & ((1 << 63) - 1))
    probs = [np.exp(nd.logweights - _logsumexp(nd.logweights)) for nd in nodes]
    out = np.zeros((int(n_samples), len(nodes)), dtype=np.int64)
    for s in range(int(n_samples)):
        for j, p in enumerate(probs):
            out[s, j] = stream.categorical(p)
    return nodes, out


def _mixture_leaf_of_rows(root, xt, nodes, choice):
    """The leaf every row of `xt` falls into when sum node nodes[j] keeps child choice[j] only (split nodes keep all children):
    the chosen leaves partition the input space."""
    pick = {id(nd): int(k) for nd, k in zip(nodes, choice)}
    leaf = np.full(xt.shape[0], -1, dtype=np.int64)

    def rec(node, rows):
        if rows.size == 0:
            return
        if node.kind == "gp":
            leaf[rows] = node.leaf
        elif node.kind == "sum":
            rec(node.children[pick[id(node)]], rows)
        else:
            ch = get_child(node, xt[rows])
            for k, c in enumerate(node.children):
                rec(c, rows[ch == k])

    rec(root, np.arange(xt.shape[0], dtype=np.int64))
    return leaf


def mixture_sample(model, xtest, n_samples, seed=0, with_noise=False):
    """`n_samples` draws of a DSMGP at the rows of `xtest`, an (n_samples, n_t) array: per draw one child of every sum node is
    chosen with probability exp(logweights) (normalised; `_mixture_choices` documents the stream), split nodes keep all their
    children, so the chosen leaves partition the input space; row r of draw s is column s of `leaf_samples(model, xtest,
    n_samples, seed, with_noise)` at the entry of r under its chosen leaf.  Host composition of the device's leaf draws: rows
    under different leaves are independent given the choice.  A GaussianProcess: `posterior_sample(..., device=True)`.  PoE, gPoE
    and rBCM raise TypeError (the reference defines no joint law for them)."""
    if isinstance(model, GaussianProcess):
        return posterior_sample(model, xtest, n_samples, seed=seed, with_noise=with_noise, device=True)
    if not isinstance(model, Model) or model.family != "dsmgp":
        raise TypeError("mixture_sample takes a DSMGP or a GaussianProcess: product-of-experts models have no joint law here")
    ptr, idx, draws, info = leaf_samples(model, xtest, n_samples, seed=seed, with_noise=with_noise)
    xt = _test_matrix(model, xtest)
    n_samples = int(n_samples)
    out = np.empty((n_samples, xt.shape[0]))
    nodes, choices = _mixture_choices(model.root, n_samples, seed)
    for s in range(n_samples):
        leaf = _mixture_leaf_of_rows(model.root, xt, nodes, choices[s])
        for l in np.unique(leaf):
            rows = np.nonzero(leaf == l)[0]
            seg = idx[ptr[l]:ptr[l + 1]]            # the leaf's routed rows, ascending
            out[s, rows] = draws[ptr[l] + np.searchsorted(seg, rows), s]
    return out


# ------------------------------------------------------------------------------------ fit

_RANK_FAILED = -(1 << 30)      # info value of every leaf of a rank whose fit raised (LAPACK's info is >= 0 here)


def _fit(model, tau):
    model._upload(tau)
    model._scores_on_device = False     # the aggregated prediction on the device belongs to the fit this one replaces
    if model.shard.world > 1 and _ctx_type(model) is hipabi.Context:
        _ = model.ctx          # every rank, also one without leaves, joins the set-up of the device exchange (collective)
    failure = None
    if len(model.shard.local) == 0:
        mll_loc, info_loc, sec = np.zeros(0), np.zeros(0, dtype=np.int32), 0.0
    elif model.shard.world == 1 or model.shard.comm_ctx is not None:     # (the opt-in device exchange reads the fit's results
        model._push_hyper()                                              # in HBM: nothing to send for a fit that raised)
        mll_loc, info_loc, sec = model.ctx.fit()
    else:
        # One of several ranks: whatever goes wrong HERE (out of memory, a HIP error, bad hyper-parameters on this shard) must not
        # keep this rank out of the collective below while the others wait in it.  The failure travels as a sentinel in the info
        # column -- every rank learns of it from the same gather and raises; nobody is left in a later collective alone.
        try:
            model._push_hyper()
            mll_loc, info_loc, sec = model.ctx.fit()
        except Exception as e:      # noqa: BLE001
            failure = e
            mll_loc = np.full(len(model.shard.local), np.nan)
            info_loc, sec = np.full(len(model.shard.local), _RANK_FAILED, dtype=np.int32), 0.0
    cols = np.stack([mll_loc, info_loc.astype(np.float64)], axis=1)
    if model.shard.comm_ctx is not None:
        both = model.shard.fit_exchange(model.ctx, cols)     # device to device over RCCL, then one copy to the host
    else:
        both = model.shard.gather_leaf_columns(cols)         # one collective
    model.leaf_mll = np.ascontiguousarray(both[:, 0])
    model.leaf_info = both[:, 1].astype(np.int32)
    model.last_fit_seconds = sec
    if failure is not None:
        raise failure
    lost = np.flatnonzero(model.leaf_info == _RANK_FAILED)
    if lost.size:
        raise RuntimeError(f"fit failed on rank {int(model.shard.owner[lost[0]])} (its {lost.size} leaves have no result); "
                           "the error is in that rank's output")
    bad = np.flatnonzero(model.leaf_info != 0)
    if bad.size:
        raise np.linalg.LinAlgError(f"leaf {int(bad[0])}: leading minor of order {int(model.leaf_info[bad[0]])} "
                                    "is not positive definite")
    return sec


class FitSeconds(float):
    """What `fit!` returns -- the seconds of the leaf loop (`src/fit.jl:88,121`) -- carrying the census of the sharing
    decisions: `.census` = dict(full, copy, prefix, lowrank_as_full, leading_as_full, lowrank_leaves, leading_leaves)
    over the arms of the REFERENCE's fit!.  `lowrank_leaves` are the leaves whose reference result comes from its
    row-deletion arm (`src/fit.jl:174-201`; numerically defective) and is an exact factorisation here."""
    census = None


def fit(model, tau=0.05):
    """`fit!(model; τ)`: shared-Cholesky fit (copy + prefix sharing). Returns seconds (`FitSeconds`: the
    census of the sharing decisions rides on it, and stays on the model as `model.fit_census`)."""
    target = model.model if isinstance(model, GaussianProcess) else model
    out = FitSeconds(_fit(target, tau))
    out.census = target.fit_census
    return out


class AppendSeconds(float):
    """What `add_data` returns: the device seconds of the call.  `.fallback`: the new factors did not fit beside the old ones
    (DSMGP_E_NOMEM) and the grown table was fitted from scratch instead; `.stats`: `Context.append_stats()` of the call (None
    after a fallback); `.resume_stats`: `Context.resume_stats()` where the call kept the resident test set (`keep_test=True`),
    else None."""
    fallback = False
    stats = None
    resume_stats = None


def add_data(model, x_new, y_new, tau=0.05, keep_test=False):
    """Observe new rows and add them to a fitted model without refactorising it (`dsmgp_append_rows`): the step after an
    acquisition.  The rows are routed through the model's own tree (region membership (lb, ub] per split, the rule of `route`; a
    sum node sends a row to every child, a kernel vector to every GP of the region; a row beyond a split node's last threshold
    raises `DsmgpDomainError`, as `predict` does, and changes nothing), `model.x`, `model.y` and every leaf's `obs` / `nobs`
    grow, a leaf whose mean is the builder's default `ConstMean(mean(y[obs]))` gets the mean of its grown list (a user-supplied
    `meanFun` is kept), the overlap matrix is recomputed, and every leaf that received rows continues its factorisation from the
    blocks it keeps.  Sum-node weights stay as they are: `update(model)` is the caller's next step, as after `fit`.  The next
    `fit(model, tau)` re-derives the sharing decisions and uploads the leaf table, not the data.  Returns `AppendSeconds`;
    raises `LinAlgError` like `fit`.  `tau`: the sharing threshold of the fallback fit.
    `keep_test=True` (`dsmgp_add_rows_keep_test`, where the context's `append_rows` takes the keyword): the test set the context
    holds stays resident, so the next `predict` / `predict_gradients` / `prediction(..., full_cov=True)` on the same `xtest` goes
    straight to `predict_run`, which resumes `K_tn L^-T` from the block columns the call kept."""
    gp = model if isinstance(model, GaussianProcess) else None
    target = model.model if gp is not None else model
    if target.shard.world > 1:
        raise NotImplementedError("add_data on a sharded model: the multi-GPU exchange is out of scope")
    if not target._uploaded:
        raise hipabi.DsmgpError(hipabi.E_STATE, "add_data on a model that has never been fitted")
    ctx = target.ctx
    if not hasattr(ctx, "append_rows"):
        raise NotImplementedError(f"{type(ctx).__name__} has no append_rows")
    xn = np.asarray(x_new, dtype=np.float64)
    if xn.ndim == 1:
        xn = xn.reshape(1, -1) if target.x.shape[1] > 1 else xn.reshape(-1, 1)
    yn = np.atleast_1d(np.asarray(y_new, dtype=np.float64))
    if xn.ndim != 2 or xn.shape[1] != target.x.shape[1] or yn.shape != (xn.shape[0],) or xn.shape[0] < 1:
        raise ValueError(f"new rows of shape {xn.shape} / {yn.shape}: the model holds D = {target.x.shape[1]} columns")
    if not np.all(np.isfinite(yn)):
        raise ValueError("non-finite value in y_new")
    m, N0 = xn.shape[0], target.x.shape[0]
    if target.root.kind == "gp":
        if not np.all(np.isfinite(xn)):
            raise ValueError("non-finite value in x_new")
        ptr, idx = np.array([0, m], dtype=np.int64), np.arange(m, dtype=np.int64)
    else:
        try:
            ptr, idx = route(target.root, xn)
        except ValueError as e:
            if "outside the region" in str(e):
                raise hipabi.DsmgpDomainError(hipabi.E_DOMAIN, str(e)) from None
            raise
    y_all = np.concatenate([target.y, yn])
    grown, means = [], []
    for l, lf in enumerate(target.leaves):
        add = idx[ptr[l]:ptr[l + 1]]
        obs = np.concatenate([lf.obs, N0 + add]).astype(np.int64) if add.size else lf.obs
        grown.append(obs)
        default = getattr(lf.mean, "default", False) and add.size
        means.append(float(np.mean(y_all[obs])) if default else float(lf.mean.m))

    keeps = bool(keep_test) and "keep_test" in inspect.signature(ctx.append_rows).parameters

    def commit(keep_routes=False):
        target.x = np.asfortranarray(np.vstack([target.x, xn]))
        target.y = y_all
        for lf, obs, mu in zip(target.leaves, grown, means):
            if obs is not lf.obs:
                lf.obs, lf.nobs = obs, int(obs.size)
                if getattr(lf.mean, "default", False):
                    lf.mean = ConstMean(mu, default=True)
        if target.D is not None:
            target.D = get_overlap(target.root, target.L)
        if gp is not None:
            gp.N = int(target.x.shape[0])
        if not keep_routes:
            target._route_cache = None
        target._scores_on_device = False
        target._schedule = None          # the next fit re-derives the sharing decisions and uploads the leaf table (not the data)

    try:
        mll_, info, sec = ctx.append_rows(xn, yn, ptr, idx, means, keep_test=True) if keeps else ctx.append_rows(xn, yn, ptr, idx, means)
    except hipabi.DsmgpError as e:
        if e.code != hipabi.E_NOMEM:
            raise
        commit()
        target._uploaded = False         # whatever the context still holds: the fallback uploads everything again
        out = AppendSeconds(_fit(target, tau))
        out.fallback = True
        return out
    commit(keep_routes=keeps)
    target.leaf_mll = np.ascontiguousarray(mll_, dtype=np.float64)
    target.leaf_info = np.asarray(info, dtype=np.int32)
    target.last_fit_seconds = sec
    out = AppendSeconds(sec)
    out.stats = ctx.append_stats() if hasattr(ctx, "append_stats") else None
    if keeps:
        # the routes of the test rows are what they were (the tree did not change); `uploaded` as the context left it
        out.resume_stats = ctx.resume_stats()
        if target._route_cache is not None and out.resume_stats["test_set_dropped"]:
            target._route_cache["uploaded"] = False
    bad = np.flatnonzero(target.leaf_info != 0)
    if bad.size:
        raise np.linalg.LinAlgError(f"leaf {int(bad[0])}: leading minor of order {int(target.leaf_info[bad[0]])} "
                                    "is not positive definite")
    return out


def fit_naive(model):
    """`fit_naive!`: one full factorisation per leaf (`src/fit.jl:294-304`)."""
    target = model.model if isinstance(model, GaussianProcess) else model
    return _fit(target, None)


# ------------------------------------------------------------------------------------ mll / weights

def mll(model):
    """Tree log marginal likelihood (`src/optimize.jl:18-25`)."""
    if isinstance(model, GaussianProcess):
        return float(model.model.leaf_mll[0])
    return float(model.tindex.bottom_up(model.leaf_mll, posterior=None)[0])


def _mll_recursive(model):
    """The literal recursion of `src/optimize.jl:18-25` (cross-check of TreeIndex.bottom_up in the CPU tests)."""

    def rec(node):
        if node.kind == "gp":
            return float(model.leaf_mll[node.leaf])
        if node.kind == "split":
            return sum(rec(c) for c in node.children)
        K = len(node.children)
        return float(_logsumexp(np.array([-np.log(K) + rec(c) for c in node.children])))

    return rec(model.root)


def mll_table(model):
    """`mll!(spn, L)`: value per node id (`src/optimize.jl:27-39`)."""
    return _value_table(model, model.leaf_mll)


def _value_table(model, leaf_values):
    """The recursion of `mll!(spn, L)` over any per-leaf values (log marginals, LOO densities): value per node id."""
    tab = {}

    def rec(node):
        if node.kind == "gp":
            v = float(leaf_values[node.leaf])
        elif node.kind == "split":
            v = sum(rec(c) for c in node.children)
        else:
            K = len(node.children)
            v = float(_logsumexp(np.array([-np.log(K) + rec(c) for c in node.children])))
        tab[node.id] = v
        return v

    rec(model.root)
    return tab


def update(model):
    """`update!(model)`: posterior sum-node weights (`src/common.jl:323-334`). Returns the root value."""
    return float(model.tindex.bottom_up(model.leaf_mll, posterior="all")[0])


def _update_recursive(model):
    """The literal recursion of `src/common.jl:323-334` (cross-check of the level-order pass in the CPU tests)."""

    def rec(node):
        if node.kind == "gp":
            return float(model.leaf_mll[node.leaf])
        if node.kind == "split":
            return sum(rec(c) for c in node.children)
        K = len(node.children)
        lw = np.array([-np.log(K) + rec(c) for c in node.children])
        z = float(_logsumexp(lw))
        node.logweights = lw - z
        return z

    return rec(model.root)


def infer(model):
    """`infer!(model)` (`src/common.jl:336-355`): only sums over GPs keep posterior weights."""
    return float(model.tindex.bottom_up(model.leaf_mll, posterior="gps")[0])


def reset_weights(model):
    """`reset_weights!` (`src/common.jl:357-363`)."""
    for n in ordered_nodes(model.root):
        if n.kind == "sum":
            n.logweights[:] = -np.log(len(n.children))


# ------------------------------------------------------------------------------------ parameters

def getparams(model):
    """Concatenated log-scale hyper-vector per kernel id: [logl..., logs, logNoise]."""
    return np.concatenate([np.concatenate([lf.kernel.loghyp(), [lf.logNoise]]) for lf in model.kernel_table()])


def setparams(model, hyp):
    """`setparams!(spn, hyp)` (`src/optimize.jl:188-198`, `src/gaussianprocess.jl:153-161`)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    tab = model.kernel_table()
    c = 0
    chunks = {}
    for lf in tab:
        n = lf.kernel.nparams() + 1
        chunks[lf.kernelid] = hyp[c:c + n]
        c += n
    if c != hyp.size:
        raise ValueError(f"hyper-vector has {hyp.size} entries, model needs {c}")
    for lf in model.leaves:
        h = chunks[lf.kernelid]
        lf.logNoise = float(h[-1])
        lf.kernel.set_loghyp(h[:-1])


# ------------------------------------------------------------------------------------ gradients / training

def _check_objective(objective):
    if objective not in ("mll", "loo"):
        raise ValueError(f"objective must be 'mll' or 'loo', not {objective!r}")


def updategradients(model, active=None, objective="mll"):
    """`updategradients!(spn)` (`src/fit.jl:306-311`): per-leaf gradient vectors in the reference's order
    [dl..., ds, dnoise] (`src/gaussianprocess.jl:212-214`; [dl..., da, ds, dnoise] for the rational quadratic kernels), computed on the device for the local leaves and
    gathered.  Also stored on the leaves (kernel.dl / kernel.ds / dnoise) like the reference does.
    `active` (one flag per leaf, default all): only those leaves' gradients are computed, the other rows are zero --
    what `finetune!` needs, whose pass for leaf j weights leaf l's gradient by the overlap D[j, l] (`src/optimize.jl:101`).
    The gradients stored on the leaves (kernel.dl / kernel.ds / dnoise) are ZERO outside the active set, where the reference
    stores every leaf's gradient on every pass (they are multiplied by D[j, l] = 0 there and never read otherwise); the
    streaming context ignores the mask and computes all of them.
    `objective="loo"`: the rows are the true derivatives of each leaf's LOO log predictive density (`dsmgp_loo_gradients`, GPML
    eq. 5.13) instead, and the densities themselves are stored in `leaf_lpd` (what `loo_objective` and `grad_loo` read); no mask
    (`active` must be None), no streaming context."""
    _check_objective(objective)
    target = model.model if isinstance(model, GaussianProcess) else model
    stride = max(lf.kernel.nparams() + 1 for lf in target.leaves)
    if objective == "loo":
        if active is not None:
            raise ValueError("updategradients: the LOO gradients take no mask")
        if len(target.shard.local):
            g_loc, lpd_loc = target.ctx.loo_gradients(stride)
        else:
            g_loc, lpd_loc = np.zeros((0, stride)), np.zeros(0)
        g = target.shard.gather_leaf_columns(g_loc[:, :stride])
        target.leaf_lpd = target.shard.gather_leaf_columns(lpd_loc[:, None])[:, 0]
    else:
        if len(target.shard.local) and (active is not None or getattr(target, "_grad_masked", False)):
            target.ctx.set_gradient_leaves(None if active is None else np.asarray(active)[target.shard.local])
            target._grad_masked = active is not None
        g_loc = target.ctx.gradients(stride) if len(target.shard.local) else np.zeros((0, stride))
        g = target.shard.gather_leaf_columns(g_loc[:, :stride])
    for lf, row in zip(target.leaves, g):
        n = lf.kernel.nparams()
        if lf.kernel.kind == KIND_ISO_LINEAR:
            lf.kernel.dl = float(row[0])
        elif lf.kernel.kind == KIND_ARD_LINEAR:       # [dl_1..dl_D, 0, dnoise]: no variance gradient
            lf.kernel.dl = row[: n - 1].copy()
        elif lf.kernel.kind in (KIND_ISO_RQ, KIND_ARD_RQ):       # [dl..., da, ds, dnoise]: the shape sits before the variance
            lf.kernel.dl = row[: n - 2].copy() if lf.kernel.kind == KIND_ARD_RQ else float(row[0])
            lf.kernel.da = float(row[n - 2])
            lf.kernel.ds = float(row[n - 1])
        else:
            ard = lf.kernel.kind in (KIND_ARD_SE, KIND_ARD_SE_PRODUCT, KIND_ARD_MATERN32, KIND_ARD_MATERN52)
            lf.kernel.dl = row[: n - 1].copy() if ard else float(row[0])
            lf.kernel.ds = float(row[n - 1])
        lf.dnoise = float(row[n])
    target.leaf_grad = g
    return g


def grad_mll(model, leaf_weights=None):
    """`∇mll!(spn, 0.0, 0.0, L, L[root], grad)` (`src/optimize.jl:42-89`): gradient of the tree log marginal
    w.r.t. the shared hyper-vector (concatenated per kernel id under sums over GPs).  With `leaf_weights` (one factor
    per leaf: a row of the overlap matrix) it is the `finetune!` variant, `src/optimize.jl:91-150`."""
    if isinstance(model, GaussianProcess):
        return model.model.leaf_grad[0][: model.node.kernel.nparams() + 1].copy()
    return _grad_tree(model, mll_table(model), leaf_weights)


def loo_objective(model, lpd=None):
    """The tree recursion of `mll(model)` with each leaf's LOO log predictive density in place of its log marginal (sum nodes:
    log-sum-exp with their uniform weights; split nodes: sum); for a `GaussianProcess` its density.  `lpd` (one value per leaf):
    default the densities of the current fit from the device (`ctx.loo()`), which are also stored in `leaf_lpd`."""
    target = model.model if isinstance(model, GaussianProcess) else model
    if lpd is None:
        lpd_loc = target.ctx.loo()[2] if len(target.shard.local) else np.zeros(0)
        lpd = target.leaf_lpd = target.shard.gather_leaf_columns(lpd_loc[:, None])[:, 0]
    if isinstance(model, GaussianProcess):
        return float(lpd[0])
    return _value_table(model, lpd)[model.root.id]


def grad_loo(model):
    """Gradient of `loo_objective(model)` w.r.t. the shared hyper-vector: the recursion of `grad_mll` on the table of the LOO
    densities `leaf_lpd` and the leaf gradients `leaf_grad`, both left by `updategradients(model, objective="loo")`.  It is the
    true gradient of that objective (`_grad_tree(rho=False)`): a sum node of K children weighs child c by
    exp(-log K + value_c - value_node), where `∇mll!` multiplies by K again under a sum over split nodes and leaves the 1 / K
    out under a sum over GPs."""
    if isinstance(model, GaussianProcess):
        return model.model.leaf_grad[0][: model.node.kernel.nparams() + 1].copy()
    return _grad_tree(model, _value_table(model, model.leaf_lpd), None, rho=False)


def _grad_tree(model, tab, leaf_weights, rho=True):
    """`∇mll!` over a table of node values `tab` and the per-leaf gradients `model.leaf_grad` (shared by grad_mll and grad_loo).
    `rho=False`: every sum node of K children weighs a child by exp(-log K + child - node) and nothing else -- without the
    reference's `+ log K` (`src/optimize.jl:70-73`) and with the `-log K` it leaves out under a sum over GPs (`:76-89`): the true
    derivative of the root value.  Two parts: the scalar weight of every leaf (`_tree_leaf_weights`), then the scatter of the
    weighted leaf rows into the hyper-vector (`_scatter_leaf_rows`)."""
    visits = _tree_leaf_weights(model, tab, leaf_weights, rho)
    return _scatter_leaf_rows(model, model.leaf_grad, visits)


def _tree_leaf_weights(model, tab, leaf_weights=None, rho=True):
    """The scalar weight of every leaf in `∇mll!` over the node values `tab`: a list of `(leaf, weight, offset, size)` in the
    order the recursion visits the leaves, `offset` / `size` the slice of the hyper-vector the leaf's row is added to."""
    logS = tab[model.root.id]
    n_hyp = getparams(model).size
    visits = []

    def rec(node, dparent, lrho, off, size):
        if node.kind == "gp":
            w = np.exp(-logS + lrho + tab[node.id] + dparent)                 # :48
            if leaf_weights is not None:
                w = w * leaf_weights[node.leaf]                               # :101
            visits.append((node.leaf, w, off, size))
        elif node.kind == "split":
            for c in node.children:
                rec(c, dparent + (tab[node.id] - tab[c.id]), lrho, off, size)  # :58-61
        elif node.of_gps:
            c0 = 0
            for c in node.children:                                           # :76-89
                nn = c.kernel.nparams() + 1
                lo = min(off + c0, off + size)
                rec(c, dparent if rho else dparent - np.log(len(node.children)), lrho, lo, min(off + c0 + nn, off + size) - lo)
                c0 += nn
        else:
            K = len(node.children)
            for c in node.children:
                rec(c, -np.log(K) + dparent, np.log(K) + lrho if rho else lrho, off, size)   # :70-73

    rec(model.root, 0.0, 0.0, 0, n_hyp)
    return visits


def _scatter_leaf_rows(model, rows, visits):
    """`grad[offset : offset + size] += rows[leaf][:size] * weight` for every visit, in order (`src/optimize.jl:49`)."""
    grad = np.zeros(getparams(model).size)
    for leaf, w, off, size in visits:
        g = grad[off:off + size]
        g += rows[leaf][: g.size] * w                                         # :49
    return grad


def targets_objective(model):
    """`sum_q` of the tree recursion of `mll(model)` over column `q` of the `(L, Q)` table the last `fit_targets` returned:
    `sum_q log p_tree(Y[:, q])`; for a `GaussianProcess` the sum of its row."""
    target = model.model if isinstance(model, GaussianProcess) else model
    tab = getattr(target, "targets_mll", None)
    if tab is None:
        raise hipabi.DsmgpError(hipabi.E_STATE, "targets_objective before fit_targets")
    if isinstance(model, GaussianProcess):
        return float(np.sum(tab[0]))
    return float(sum(_value_table(model, tab[:, q])[model.root.id] for q in range(tab.shape[1])))


def targets_weight_table(model):
    """The `(L, Q)` table of `grad_targets`: entry `[l, q]` is the weight `∇mll!` gives leaf `l` when column `q` of the last
    `fit_targets` table stands for the leaf log marginals."""
    target = model.model if isinstance(model, GaussianProcess) else model
    tab = target.targets_mll
    if isinstance(model, GaussianProcess):
        return np.ones_like(tab), [(0, 1.0, 0, model.node.kernel.nparams() + 1)]
    W = np.zeros_like(tab)
    visits = []
    for q in range(tab.shape[1]):
        visits = _tree_leaf_weights(model, _value_table(model, tab[:, q]))
        for leaf, w, _, _ in visits:
            W[leaf, q] += w
    return W, visits


def grad_targets(model):
    """Gradient of `targets_objective(model)` w.r.t. the shared hyper-vector in `grad_mll`'s convention (the reference's
    `∇mll!`, column by column): with `Y = y[:, None]` it equals `grad_mll(model)`.  The weight of every (leaf, column) comes from
    the tree recursion on that column's table; ONE device call returns `sum_q W[l, q] dmll[l, q] / dtheta` per leaf
    (`Context.targets_gradients`: one inversion and one contraction per leaf whatever Q is), and the rows are scattered into
    the hyper-vector with weight 1.  Needs `fit_targets` on the current fit."""
    target = _targets_model(model, "grad_targets")
    if getattr(target, "targets_mll", None) is None:
        raise hipabi.DsmgpError(hipabi.E_STATE, "grad_targets before fit_targets")
    W, visits = targets_weight_table(model)
    stride = max(lf.kernel.nparams() + 1 for lf in target.leaves)
    rows = target.ctx.targets_gradients(stride, W)
    target.targets_leaf_grad = rows
    if isinstance(model, GaussianProcess):
        return rows[0][: model.node.kernel.nparams() + 1].copy()
    return _scatter_leaf_rows(model, rows, [(leaf, 1.0, off, size) for leaf, _, off, size in visits])


def loo_targets(model):
    """Leave-one-out cross-validation of every leaf GP under every column of the last `fit_targets` (`dsmgp_loo_columns`), on the
    one factorisation: dict(obs, mu, var, lpd) like `loo(model)`, with `mu[l]` of shape `(n_l, Q)`, `var[l]` of length `n_l` (the
    same for every column) and `lpd` of shape `(L, Q)`, which is also stored in `targets_lpd`.  Needs `fit_targets` on the
    current fit; streaming and multi-rank models refuse as `fit_targets` does."""
    target = _targets_model(model, "loo_targets")
    if getattr(target, "targets_mll", None) is None:
        raise hipabi.DsmgpError(hipabi.E_STATE, "loo_targets before fit_targets")
    mu, var, lpd = target.ctx.loo_targets()
    target.targets_lpd = np.ascontiguousarray(lpd)
    ptr, idx = obs_table(target.leaves)
    return dict(obs=[np.asarray(idx[ptr[l]:ptr[l + 1]], dtype=np.int64) for l in range(target.L)],
                mu=[mu[ptr[l]:ptr[l + 1]] for l in range(target.L)],
                var=[var[ptr[l]:ptr[l + 1]] for l in range(target.L)], lpd=target.targets_lpd.copy())


def loo_targets_objective(model, lpd=None):
    """`sum_q` of the recursion of `loo_objective` on column `q` of the `(L, Q)` table of LOO densities: default the table of
    the current fit from the device (`loo_targets`), which is also stored in `targets_lpd`; for a `GaussianProcess` the sum of
    its row."""
    target = model.model if isinstance(model, GaussianProcess) else model
    if lpd is None:
        lpd = loo_targets(model)["lpd"]
    lpd = np.asarray(lpd, dtype=np.float64)
    if isinstance(model, GaussianProcess):
        return float(np.sum(lpd[0]))
    return float(sum(_value_table(target, lpd[:, q])[target.root.id] for q in range(lpd.shape[1])))


def grad_loo_targets(model):
    """The true gradient of `loo_targets_objective(model)` w.r.t. the shared hyper-vector; with `Y = y[:, None]` it is
    `grad_loo(model)`.  The weight of every (leaf, column) comes from `_tree_leaf_weights(..., rho=False)` on that column of the
    table of LOO densities (exponentials: non-negative, as the device call requires); ONE device call returns
    `sum_q W[l, q] dlpd[l, q] / dtheta` per leaf (`Context.loo_targets_gradients`: one inverse and one contraction per leaf
    whatever Q is), and the rows are scattered into the hyper-vector with weight 1.  The table the call returns is stored in
    `targets_lpd`.  Needs `fit_targets` on the current fit."""
    target = _targets_model(model, "grad_loo_targets")
    if getattr(target, "targets_mll", None) is None:
        raise hipabi.DsmgpError(hipabi.E_STATE, "grad_loo_targets before fit_targets")
    stride = max(lf.kernel.nparams() + 1 for lf in target.leaves)
    if isinstance(model, GaussianProcess):
        rows, lpd = target.ctx.loo_targets_gradients(stride)
        target.targets_lpd = np.ascontiguousarray(lpd)
        return rows[0][: model.node.kernel.nparams() + 1].copy()
    tab = getattr(target, "targets_lpd", None)
    if tab is None:
        tab = loo_targets(model)["lpd"]
    W = np.zeros_like(tab)
    visits = []
    for q in range(tab.shape[1]):
        visits = _tree_leaf_weights(target, _value_table(target, tab[:, q]), None, rho=False)
        for leaf, w, _, _ in visits:
            W[leaf, q] += w
    rows, lpd = target.ctx.loo_targets_gradients(stride, W)
    target.targets_lpd = np.ascontiguousarray(lpd)
    return _scatter_leaf_rows(target, rows, [(leaf, 1.0, off, size) for leaf, _, off, size in visits])


class ADAM:
    """Flux.Optimise.ADAM stand-in for `train!`.  With stateful=False (default) the moment estimates are
    reset every step, which is what the reference effectively runs: `hyp += grad` rebinds `hyp`, so Flux's
    IdDict-keyed state never carries over and the step is eta*g/(|g|+eps) (`src/optimisers.jl:78-79`,
    SURVEY F9).  stateful=True is the textbook optimiser."""

    def __init__(self, eta=1e-3, beta=(0.9, 0.999), eps=1e-8, stateful=False):
        self.eta, self.beta, self.eps, self.stateful = eta, beta, eps, stateful
        self.m = self.v = None
        self.t = 0

    def apply(self, x, g):
        if not self.stateful or self.m is None:
            self.m = np.zeros_like(g)
            self.v = np.zeros_like(g)
            self.t = 0
        b1, b2 = self.beta
        self.t += 1
        self.m = b1 * self.m + (1 - b1) * g
        self.v = b2 * self.v + (1 - b2) * g * g
        return self.m / (1 - b1 ** self.t) / (np.sqrt(self.v / (1 - b2 ** self.t)) + self.eps) * self.eta


class RMSProp:
    """Flux.Optimise.RMSProp stand-in (default optimiser of `train!(gp)`, `src/optimisers.jl:91`); stateful=False
    restarts the running average every step, which is what the reference's rebinding `hyp += grad` amounts to
    (SURVEY F9): the step is eta * g / (sqrt(1 - rho) |g| + eps)."""

    def __init__(self, eta=1e-3, rho=0.9, eps=1e-8, stateful=False):
        self.eta, self.rho, self.eps, self.stateful = eta, rho, eps, stateful
        self.acc = None

    def apply(self, x, g):
        if not self.stateful or self.acc is None:
            self.acc = np.zeros_like(g)
        self.acc = self.rho * self.acc + (1 - self.rho) * g * g
        return g * (self.eta / (np.sqrt(self.acc) + self.eps))


def _train_gp(gp, optim, iterations, lam, randinit, seed, verbose, objective="mll", targets=None, targets_objective_kind="mll"):
    """`train!(gp::GaussianProcess; iterations, optim, λ)` (`src/optimisers.jl:89-145`): ascent on one GP's log
    marginal; a NaN log marginal (or a factorisation that fails: LAPACK info > 0, which the reference's potrf! call
    ignores and which then shows up as NaN) rolls back to the previous hyper-vector and returns; early stop when the
    last value is within λ of the mean of the nine before it (`:118`, a single hit suffices here)."""
    from .datagen import normal
    target = gp.model
    n = getparams(target).size
    hyp = normal(seed, 0, n) if randinit else getparams(target).copy()
    old = hyp.copy()
    hist = []
    for it in range(1, iterations + 1):
        setparams(target, hyp)
        try:
            update_cholesky(gp)
            ell = mll(gp)
        except (np.linalg.LinAlgError, ValueError, hipabi.DsmgpError):   # failed potrf / non-finite hyper-parameters
            ell = float("nan")
        if objective == "loo" and not np.isnan(ell):      # value and gradient from one call, outside the try: an error of the
            updategradients(gp, objective="loo")          # LOO pass itself (memory, ArdSE with D > 35) is an error, as for the
            ell = loo_objective(gp, lpd=gp.model.leaf_lpd)    # marginal-likelihood gradients below
        if targets is not None and not np.isnan(ell):     # sum_q mll of the target columns on this factorisation
            fit_targets(gp, targets)
            ell = loo_targets_objective(gp) if targets_objective_kind == "loo" else targets_objective(gp)
        hist.append(ell)
        if np.isnan(ell):                                                     # :115-119
            setparams(target, old)
            update_cholesky(gp)
            return gp, np.array(hist)
        delta = abs(ell - np.mean(hist[-10:-1])) if it > 10 else np.inf        # :121
        if verbose:
            print(f"iter {it}: {objective} {ell:.6f} delta {delta:.3g}")
        if delta < lam:                                                       # :125-128
            return gp, np.array(hist)
        if objective == "loo":
            g = grad_loo(gp)
        elif targets is not None:
            g = grad_loo_targets(gp) if targets_objective_kind == "loo" else grad_targets(gp)
        else:
            updategradients(gp)
            g = grad_mll(gp)
        old = hyp.copy()
        hyp = hyp + optim.apply(hyp, g)                                       # :135-137 (ascent)
    setparams(target, hyp)
    update_cholesky(gp)
    return gp, np.array(hist)


def train(model, optim=None, *, iterations=10_000, lam=None, randinit=True, earlystop=10, seed=0, tau=0.05, verbose=False,
          objective="mll", targets=None, targets_objective="mll"):
    """`train!(model, optim; iterations, λ, randinit, earlystop)` (`src/optimisers.jl:4-87`): gradient ASCENT
    on the tree log marginal over one shared hyper-vector.  Returns (model, history of root mll).
    For a single `GaussianProcess` it is `train!(gp; iterations, optim, λ)` (`src/optimisers.jl:89-145`:
    RMSProp, λ = 0.1, rollback on a NaN log marginal).
    `objective="loo"`: the same loops on `loo_objective(model)` -- history and early stop on it, ascent on `grad_loo` (no
    counterpart in the reference); a streaming model refuses (`DsmgpError`, E_STATE).
    `targets=Y` (`(N, Q)`, default None: nothing changes): the same loops on `targets_objective(model)`, one kernel trained on all
    Q columns -- per iteration `setparams`, `fit`, `fit_targets`, `grad_targets`, optimiser step.  Not together with
    `objective="loo"`; streaming and multi-rank models refuse as `fit_targets` does.
    `targets_objective="loo"` (with `targets=Y`; default "mll": nothing changes): the loops run on `loo_targets_objective(model)`
    instead, the summed leave-one-out densities of the columns, with `grad_loo_targets` as the gradient.  Any other value raises
    `ValueError`."""
    from .datagen import normal
    _check_objective(objective)
    if targets_objective not in ("mll", "loo"):
        raise ValueError(f"targets_objective must be 'mll' or 'loo', not {targets_objective!r}")
    if targets is not None:
        if objective == "loo":
            raise ValueError("train: targets go with the marginal likelihood objective, not with objective='loo'")
        _targets_model(model, "train(targets=...)")
    if isinstance(model, GaussianProcess):
        return _train_gp(model, RMSProp() if optim is None else optim, iterations, 0.1 if lam is None else lam, randinit, seed,
                         verbose, objective, targets, targets_objective)
    has_leaves = len(model.shard.local) > 0
    # factor-and-discard context: a pass over the leaf groups cannot be revisited, so the loop's fit! asks for the
    # gradients of the same pass up front (one pass per iteration instead of a fit pass plus a fit + gradient pass)
    streaming = has_leaves and hasattr(model.ctx, "want_gradients")
    if streaming and objective == "loo":
        raise hipabi.DsmgpError(hipabi.E_STATE, "train: the LOO objective needs the factors of a resident Context; a streaming "
                                                "pass discards them with their leaf group")
    lam = 0.05 if lam is None else lam
    optim = ADAM() if optim is None else optim
    n = getparams(model).size
    hyp = normal(seed, 0, n) if randinit else getparams(model)
    hist = []
    c = 0
    if has_leaves:
        model.ctx.set_joint(False)     # fit is not followed by predict inside the loop: keep resident test rows out of it
    if streaming:
        model.ctx.want_gradients = max(lf.kernel.nparams() + 1 for lf in model.leaves)
        model.ctx.groups = None
    try:
        return _train_loop(model, optim, hyp, hist, c, iterations, lam, earlystop, tau, verbose, streaming, objective, targets,
                           targets_objective)
    finally:
        if streaming:                  # also after an error inside the loop: later passes must not collect gradients
            model.ctx.want_gradients = 0
            model.ctx.groups = None
        if has_leaves:
            model.ctx.set_joint(True)


def _train_loop(model, optim, hyp, hist, c, iterations, lam, earlystop, tau, verbose, streaming=False, objective="mll",
                targets=None, targets_objective_kind="mll"):
    def plain_fits():
        if streaming:                  # the fits after the loop need no gradients: smaller groups, fewer passes
            model.ctx.want_gradients = 0
            model.ctx.groups = None

    for it in range(1, iterations + 1):
        setparams(model, hyp)
        fit(model, tau=tau)
        if objective == "loo":          # value and gradient from one call
            updategradients(model, objective="loo")
            ell = loo_objective(model, lpd=model.leaf_lpd)
        elif targets is not None:
            fit_targets(model, targets)
            ell = loo_targets_objective(model) if targets_objective_kind == "loo" else targets_objective(model)
        else:
            ell = mll(model)
        hist.append(ell)
        delta = abs(ell - np.mean(hist[-10:-1])) if it > 10 else np.inf       # :53
        c = c + 1 if delta < lam else 0
        if verbose:
            print(f"iter {it}: {objective} {ell:.6f} delta {delta:.3g}")
        if c >= earlystop:
            plain_fits()
            return model, np.array(hist)
        if objective == "loo":
            g = grad_loo(model)
        elif targets is not None:
            g = grad_loo_targets(model) if targets_objective_kind == "loo" else grad_targets(model)
        else:
            updategradients(model)
            g = grad_mll(model)
        hyp = hyp + optim.apply(hyp, g)                                       # :78-79 (ascent)
    plain_fits()
    setparams(model, hyp)
    fit(model, tau=tau)
    return model, np.array(hist)


def _overlap_row(D, j):
    return D.row(j) if hasattr(D, "row") else np.asarray(D[j, :], dtype=np.float64)


def finetune(model, optim=None, *, iterations=1000, lam=0.5, tau=0.05, verbose=False):
    """`finetune!(model, optim; iterations, λ)` (`src/finetuning.jl:3-87`): one hyper-vector PER LEAF.  Every
    iteration visits every leaf j: all leaves are set to leaf j's vector, the whole tree is refitted, and leaf j's
    vector takes an ascent step along the tree gradient in which leaf l's contribution is weighted by the overlap
    D[j, l] (`src/optimize.jl:91-150`; the diagonal of D is zero, so the leaf's own term does not enter -- the
    reference passes `D` at `:54`, not the `Dd` it prepares at `:30-31`).  That is L whole-tree fit! +
    updategradients! passes per iteration, each one batched call here.  The history is the sum over leaves of each
    leaf's own log marginal at its own vector (`:51,59`); early stopping as `:61-79`.  At the end every leaf keeps
    its own vector: the leaves get kernel ids of their own and are refactorised (`:74-77,82-85`).  One kernel id only: the reference's
    `setparams!(spn, hyp_)` with a single leaf's vector is ill-formed for kernel vectors."""
    if len(model.kernel_table()) != 1:
        raise NotImplementedError("finetune: models with a kernel vector are not supported (ill-formed in the reference)")
    optim = ADAM() if optim is None else optim
    L = model.L
    hyp = [np.concatenate([lf.kernel.loghyp(), [lf.logNoise]]) for lf in model.leaves]
    rows = [_overlap_row(model.D, j) for j in range(L)]
    hist, c = [], 0
    model.ctx.set_joint(False)
    try:
        for it in range(1, iterations + 1):
            ell = 0.0
            for j, lf in enumerate(model.leaves):
                setparams(model, hyp[j])
                fit(model, tau=tau)
                updategradients(model, active=rows[j] != 0)       # every other leaf's term is multiplied by D[j, l] = 0
                ell += float(model.leaf_mll[lf.leaf])                             # :51
                hyp[j] = hyp[j] + optim.apply(hyp[j], grad_mll(model, leaf_weights=rows[j]))   # :54-56
            hist.append(ell)
            delta = abs(ell - np.mean(hist[-10:-1])) if it > 10 else np.inf          # :61
            c = c + 1 if delta < lam else 0
            if verbose:
                print(f"iter {it}: sum of leaf mll {ell:.6f} delta {delta:.3g}")
            if c >= 10:
                break
    finally:
        model.ctx.set_joint(True)
        if getattr(model, "_grad_masked", False) and len(model.shard.local):
            model.ctx.set_gradient_leaves(None)
            model._grad_masked = False
    # every leaf keeps its own hyper-parameters: a kernel id per leaf, then one factorisation each (:74-77, :82-85)
    before = [(lf.kernelid, lf.logNoise, lf.kernel.loghyp().copy()) for lf in model.leaves]
    for j, lf in enumerate(model.leaves):
        lf.kernelid = j
        lf.logNoise = float(hyp[j][-1])
        lf.kernel.set_loghyp(hyp[j][:-1])
    model._ktab = None
    model._uploaded = False
    try:
        fit_naive(model)
    except Exception:
        # leave the model as it was before the per-leaf ids were assigned (one shared vector, refittable)
        for lf, (kid, ln, lh) in zip(model.leaves, before):
            lf.kernelid, lf.logNoise = kid, ln
            lf.kernel.set_loghyp(lh)
        model._ktab = None
        model._uploaded = False
        raise
    return model, np.array(hist)


# ------------------------------------------------------------------------------------ predict

def _content_hash(a):
    """64-bit hash of an array's contents: what tells `predict` that it is handed the test set it has registered (the cache key
    is (shape, this hash): a 64-bit content hash decides whether the rows are registered again -- a collision between two test
    matrices of one shape would reuse the first one's routes, at odds of 2^-64 per pair).  xxh3 over the array's own buffer in
    whichever contiguous layout it has -- `predict` hands over Fortran-ordered matrices (the layout of the C ABI), whose buffer
    is the C-ordered buffer of the transpose; anything else (a strided slice) is hashed through one contiguous copy.  xxhash is
    an optional dependency: without it the bytes go through Python's own hash (a copy and a SipHash: 0.65 ms for 10k x 8 rows
    against 0.03 ms)."""
    if a.flags.c_contiguous:
        buf = a
    elif a.flags.f_contiguous:
        buf = a.T
    else:
        buf = np.ascontiguousarray(a)
    if a.size == 0:
        return 0
    if _xxhash is not None:
        return _xxhash.xxh3_64_intdigest(memoryview(buf).cast("B"))
    return hash(buf.tobytes())


def _routing(model, xt, host_routes=True):
    """Routes of one test set, cached on the model: which rows each leaf predicts (CSR over all leaves and over
    this rank's leaves) and, filled lazily by the aggregation, the child masks of every split node.  With
    host_routes=False only the cache entry is made: the context routes the rows itself (`set_test_routed`)."""
    key = (xt.shape, _content_hash(xt))
    rc = model._route_cache
    if rc is None or rc["key"] != key:
        rc = model._route_cache = dict(key=key, ptr=None, idx=None, lptr=None, lidx=None, masks={}, uploaded=False)
    if host_routes and rc["ptr"] is None:
        ptr, idx = route(model.root, xt) if model.family == "dsmgp" else route_all(model.root, xt.shape[0])
        lptr, lidx = model.shard.subset.take_csr(ptr, idx)     # (ptr, idx themselves where this rank holds every leaf)
        rc.update(ptr=ptr, idx=idx, lptr=lptr, lidx=lidx)
    return rc


def _register_rows(model, xt, rc):
    """The test rows -> the context (once per test matrix): routed on the device where the context holds the tree."""
    if rc["uploaded"]:
        return
    if model._device_routing:
        try:
            model.ctx.set_test_routed(xt)
            rc["uploaded"] = True
            return
        except hipabi.DsmgpError as e:
            # the routing workspace (bitmap + prefixes: 8 L ceil(n_t / 32) bytes) did not fit: the host lists need none of it.
            # Anything else (a row outside a split region: DsmgpDomainError, a ValueError like the host routing's) is the caller's
            if e.code != hipabi.E_NOMEM:
                raise
    if rc["ptr"] is None:
        _routing(model, xt)
    model.ctx.set_test(xt, rc["lptr"], rc["lidx"])
    rc["uploaded"] = True


def _leaf_moments(model, xt, rc):
    """(mu, var) per (leaf, routed row) for ALL leaves, computed on the owning ranks."""
    counts = np.diff(rc["ptr"])
    if len(model.shard.local) == 0:
        return model.shard.gather_ragged_pair(np.zeros(0), np.zeros(0), counts)
    if not rc["uploaded"]:
        model.ctx.set_test(xt, rc["lptr"], rc["lidx"])      # (the per-(leaf, row) moments come back aligned with THESE lists)
        rc["uploaded"] = True
    model.last_predict_seconds = model.ctx.predict_run()
    mu_l, var_l = model.ctx.predict_fetch()
    return model.shard.gather_ragged_pair(mu_l, var_l, counts)


def _test_matrix(model, xtest):
    """`xtest` as the n_t x D Fortran-ordered matrix the C ABI reads; a matrix of another width than the training data is
    refused here, on every path (device routing reads n_t * D doubles from the caller's buffer)."""
    xt = np.asfortranarray(xtest, dtype=np.float64)
    if xt.ndim == 1:
        xt = xt.reshape(-1, 1)
    if xt.ndim != 2 or xt.shape[1] != model.x.shape[1]:
        raise ValueError(f"test matrix of shape {xt.shape}: the model was trained on D = {model.x.shape[1]} columns")
    return xt


def resident_test(model, xtest, tau=0.05):
    """Register `xtest` as the resident test set BEFORE the next fit (no reference counterpart): that fit then
    carries the test rows through its factorisation launches and the following `predict(model, xtest)` only
    finishes the moments.  `predict` registers its argument by itself, which pays off from the second fit on;
    this call is for evaluation loops that know their test set up front and for the streaming context, where a
    prediction after an unprepared fit costs a second pass over all leaf groups."""
    xt = _test_matrix(model, xtest)
    if xt.shape[0] == 0:
        return                      # nothing to carry along
    model._upload(tau)
    rc = _routing(model, xt, host_routes=not model._device_routing)
    if len(model.shard.local):
        _register_rows(model, xt, rc)


def predict(model, xtest):
    """`predict(model, x)` -> (mu, var) of length n_t (`src/common.jl:294-307`).  The rows are registered with the context once per
    test matrix: whether `x` is the registered one is decided by (shape, 64-bit content hash) -- `_content_hash`.  The per-(leaf, row) moments stay on
    the device and are aggregated there (`dsmgp_aggregate*`); contexts without that entry (the streaming context, whose
    moments are on the host anyway) use the host rules below."""
    if isinstance(model, GaussianProcess):
        mu, var = prediction(model, xtest)
        var = np.where(var <= 0, EPS, var)
        return mu, var
    xt = _test_matrix(model, xtest)
    model._scores_on_device = False
    if xt.shape[0] == 0:            # no rows: (Float64[], Float64[]) as in the reference; no device call, no collective (every rank sees the same x)
        return np.zeros(0), np.zeros(0)
    if model.family == "dsmgp" and model.root.kind != "gp" and not model.tindex.weights_normalised():
        # `_predict` shifts the means by c = mu_min - 1 before it weighs them (`src/common.jl:134-143,275-302`): with weights
        # that add up to one the shift cancels and the recursion IS the flat mixture the device aggregates; with weights a
        # caller assigned by hand it leaves c (1 - sum of weights) per sum node behind.  Then: the literal recursion on the
        # host, from the per-(leaf, row) moments of the device (the same on every rank: it depends on the weights alone)
        rc = _routing(model, xt)
        mu, var = _leaf_moments(model, xt, rc)
        return _aggregate_dsmgp(model, xt, rc["ptr"], mu, var)
    if hasattr(_ctx_type(model), "aggregate_partial"):       # decided by the model's construction: the same on every rank
        # (a rank that holds leaves and whose context holds the tree routes its rows on the device: no host lists at all)
        return _predict_device(model, xt, _routing(model, xt, host_routes=not model._device_routing))
    rc = _routing(model, xt)
    mu, var = _leaf_moments(model, xt, rc)
    if model.family == "dsmgp":
        return _aggregate_dsmgp_flat(model, xt.shape[0], rc, mu, var)
    return _aggregate_poe(model, xt, rc["ptr"], mu, var)


def aggregate_input_gradients(family, mu, var, dmu, dvar, ent, coef=None, group=None, G=0, plain=False, kss_prior=None,
                              noise_prior=None, dkss_prior=None):
    """(dmu, dvar), each (n_t, D): the gradients of the aggregated prediction of one family with respect to the test point,
    from the per-entry moments `mu`, `var` (length E) and their input gradients `dmu`, `dvar` (E x D).  `ent[r]` lists the
    (leaf, entry) pairs of test row r in ascending entry order; the other arguments are those of the aggregation itself
    (`dsmgp_aggregate`: family 0 mixture, 1 PoE, 2 gPoE, 3 rBCM; `coef[l]` = W_l or beta_l, `group[l]` and `G` for rBCM, whose
    prior term is s = `kss_prior[r]` + `noise_prior` with ds/dx = `dkss_prior[r]`, zero for a stationary kernel).  Pure
    NumPy on the host; nothing is modified.
      mixture   dmu = sum W dmu_l,  dvar = sum W [dvar_l + 2 (mu_l - mu) dmu_l]  (plain: sum W dvar_l); a leaf variance the
                aggregation clamps (sigma2_l <= 0 -> 1e-8) is a constant: dvar_l = 0
      PoE/gPoE  T = sum beta / sigma2_l, P = sum beta mu_l / sigma2_l, mu = P / T, var = 1 / T:
                dT = -sum beta dvar_l / sigma2_l^2, dP = sum beta (dmu_l / sigma2_l - mu_l dvar_l / sigma2_l^2),
                dmu = (dP - mu dT) / T, dvar = -dT / T^2
      rBCM      per group g that saw the row T_g, P_g, dT_g, dP_g as above with beta = 1; beta_g = (log s + log T_g) / 2,
                dbeta_g = (ds / s + dT_g / T_g) / 2; C = 1 / s + sum_g beta_g (T_g - 1 / s), m = sum_g beta_g P_g,
                dC = -ds / s^2 + sum_g [dbeta_g (T_g - 1 / s) + beta_g (dT_g + ds / s^2)], dm = sum_g (dbeta_g P_g + beta_g dP_g),
                mu = m / C, var = 1 / C: dmu = (dm - mu dC) / C, dvar = -dC / C^2
    The tree is piecewise constant in x (which leaves see a row does not change inside a region): this is the gradient
    inside the row's region."""
    mu = np.asarray(mu, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    dmu = np.asarray(dmu, dtype=np.float64)
    dvar = np.asarray(dvar, dtype=np.float64)
    n_t = len(ent)
    D = dmu.shape[1]
    rows = np.array([r for r, er in enumerate(ent) for _ in er], dtype=np.int64)
    leaf = np.array([l for er in ent for l, _ in er], dtype=np.int64)
    e = np.array([k for er in ent for _, k in er], dtype=np.int64)
    m, v, dm, dv = mu[e], var[e], dmu[e], dvar[e]

    def rowsum(a, idx=rows, n=n_t):
        out = np.zeros((n,) + a.shape[1:])
        np.add.at(out, idx, a)
        return out

    if family == 0:
        w = np.asarray(coef, dtype=np.float64)[leaf]
        clamped = ~(v > 0)
        dv = np.where(clamped[:, None], 0.0, dv)
        s0 = rowsum(w * m)
        out_dmu = rowsum(w[:, None] * dm)
        if plain:
            return out_dmu, rowsum(w[:, None] * dv)
        return out_dmu, rowsum(w[:, None] * (dv + 2.0 * (m - s0[rows])[:, None] * dm))
    if family != 3:
        b = np.asarray(coef, dtype=np.float64)[leaf]
        t = b / v
        T = rowsum(t)
        P = rowsum(t * m)
        dT = rowsum(-(t / v)[:, None] * dv)
        dP = rowsum(t[:, None] * dm - (t * m / v)[:, None] * dv)
        mu_a = P / T
        return (dP - mu_a[:, None] * dT) / T[:, None], -dT / (T * T)[:, None]
    grp = np.asarray(group, dtype=np.int64)[leaf]
    key = rows * G + grp
    t = 1.0 / v
    T = rowsum(t, key, n_t * G).reshape(n_t, G)
    P = rowsum(t * m, key, n_t * G).reshape(n_t, G)
    dT = rowsum(-(t / v)[:, None] * dv, key, n_t * G).reshape(n_t, G, D)
    dP = rowsum(t[:, None] * dm - (t * m / v)[:, None] * dv, key, n_t * G).reshape(n_t, G, D)
    seen = np.zeros(n_t * G, dtype=bool)
    seen[key] = True
    seen = seen.reshape(n_t, G)
    s = np.asarray(kss_prior, dtype=np.float64) + float(noise_prior)
    ds = np.zeros((n_t, D)) if dkss_prior is None else np.asarray(dkss_prior, dtype=np.float64)
    Ts = np.where(seen, T, 1.0)
    beta = np.where(seen, 0.5 * (np.log(s)[:, None] + np.log(Ts)), 0.0)
    dbeta = np.where(seen[:, :, None], 0.5 * ((ds / s[:, None])[:, None, :] + dT / Ts[:, :, None]), 0.0)
    ds_s2 = ds / (s * s)[:, None]
    C = 1.0 / s + np.sum(beta * (np.where(seen, T, 0.0) - np.where(seen, 1.0, 0.0) / s[:, None]), axis=1)
    mm = np.sum(beta * P, axis=1)
    dC = -ds_s2 + np.sum(dbeta * (Ts - 1.0 / s[:, None])[:, :, None] + beta[:, :, None] * (dT + ds_s2[:, None, :]), axis=1)
    dmm = np.sum(dbeta * P[:, :, None] + beta[:, :, None] * dP, axis=1)
    mu_a = mm / C
    return (dmm - mu_a[:, None] * dC) / C[:, None], -dC / (C * C)[:, None]


def _prior_diag_grad(lf, xt):
    """d k(x, x) / dx of the leaf's kernel at the rows of `xt`: 2 x_d / l_d^2 for the linear kinds, 0 for the stationary ones."""
    k = lf.kernel
    if k.kind == KIND_ARD_LINEAR:
        return 2.0 * xt * np.exp(-2.0 * k.logl)[None, :]
    if k.kind == KIND_ISO_LINEAR:
        return 2.0 * xt / np.exp(k.logl) ** 2
    return np.zeros(xt.shape)


def _check_aggregate(what, aggregate):
    if aggregate not in ("host", "device"):
        raise ValueError(f'{what}: aggregate must be "host" or "device", not {aggregate!r}')


def predict_gradients(model, xtest, aggregate="host"):
    """(mu, var, dmu, dvar): `predict(model, xtest)` -- the same bits -- and the gradients of both moments with respect to
    the test point, `dmu`, `dvar` of shape (n_t, D), for a DSMGP, PoE, gPoE, rBCM or a single GaussianProcess (no reference
    counterpart).  The per-(leaf, row) gradients come from the device (`Context.predict_gradients`), the aggregation runs on
    the host (`aggregate_input_gradients`) or, with `aggregate="device"`, on the device (`Context.aggregate_gradients`: no
    per-entry array is fetched and no entry list is built; the result agrees with the host's to rounding, not to the bit).
    The tree is piecewise constant in x -- which leaves a row reaches changes only
    at a split threshold, where the prediction itself jumps -- so the result is the gradient inside the row's region.
    Refused: a DSMGP whose sum weights are not normalised (ValueError: `predict` then shifts the means by mu_min - 1, which
    is not differentiable), a model sharded over several ranks (NotImplementedError), and contexts that do not keep what the
    device call reads (the streaming context: DsmgpError)."""
    _check_aggregate("predict_gradients", aggregate)
    if isinstance(model, GaussianProcess):
        if aggregate == "device":       # the one-leaf table as a plain mixture (a clamped variance is a constant: dvar = 0 there)
            mu, var = predict(model, xtest)
            _, _, dmu, dvar = predict_gradients(model.model, xtest, aggregate="device")
            return mu, var, dmu, dvar
        mu, var, dmu, dvar = prediction(model, xtest, input_gradients=True)
        return mu, np.where(var <= 0, EPS, var), np.ascontiguousarray(dmu), np.ascontiguousarray(dvar)
    if model.shard.world > 1:
        raise NotImplementedError("predict_gradients: the model is sharded over several ranks; the gradients are aggregated on "
                                  "the host of a single rank only")
    if model.family == "dsmgp" and model.root.kind != "gp" and not model.tindex.weights_normalised():
        raise ValueError("predict_gradients: the sum weights are not normalised; predict then shifts the means by mu_min - 1, "
                         "which is not differentiable")
    if not hasattr(_ctx_type(model), "predict_gradients"):
        raise NotImplementedError(f"predict_gradients: {_ctx_type(model).__name__} has no predict_gradients")
    if issubclass(_ctx_type(model), hipabi.StreamingContext):
        raise hipabi.DsmgpError(hipabi.E_STATE, "predict_gradients: a streaming context discards what the input gradients read")
    xt = _test_matrix(model, xtest)
    n_t, D = xt.shape
    if n_t == 0:
        return np.zeros(0), np.zeros(0), np.zeros((0, D)), np.zeros((0, D))
    if aggregate == "device" and not hasattr(_ctx_type(model), "aggregate_gradients"):
        raise NotImplementedError(f"predict_gradients: {_ctx_type(model).__name__} has no aggregate_gradients")
    mu, var = predict(model, xt)            # routes, registers and runs as predict does; the moments stay on the device
    if aggregate == "device":               # ... and so do their sums: the gradients are reduced beside them
        _, _, _, _, plain, prior = _aggregation_spec(model)
        dmu, dvar = model.ctx.aggregate_gradients(plain=plain, prior_kernel_id=prior.kernelid if prior else 0)
        model.last_agg_gradients_seconds = model.ctx.agg_gradients_seconds
        return mu, var, np.ascontiguousarray(dmu), np.ascontiguousarray(dvar)
    rc = _routing(model, xt)                # the host's lists: entry by entry those of a context that routed the rows itself
    ptr, idx = rc["lptr"], rc["lidx"]
    mu_l, var_l = model.ctx.predict_fetch()
    dmu_l, dvar_l = model.ctx.predict_gradients()
    ent = [[] for _ in range(n_t)]
    for l in range(len(ptr) - 1):
        for k in range(int(ptr[l]), int(ptr[l + 1])):
            ent[int(idx[k])].append((l, k))
    family, coef, group, G, plain, prior = _aggregation_spec(model)
    kw = {}
    if family == hipabi.AGG_RBCM:
        kw = dict(kss_prior=_prior_diag(prior, xt), noise_prior=np.exp(2 * prior.logNoise), dkss_prior=_prior_diag_grad(prior, xt))
    dmu, dvar = aggregate_input_gradients(family, mu_l, var_l, dmu_l, dvar_l, ent, coef=coef, group=group, G=G, plain=plain, **kw)
    return mu, var, dmu, dvar


def _targets_matrix(model, Y):
    """`Y` as an (N, Q) float64 matrix over the model's training rows; a vector counts as one column."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim == 1:
        Y = Y[:, None]
    if Y.ndim != 2 or Y.shape[0] != model.x.shape[0] or Y.shape[1] < 1:
        raise ValueError(f"targets of shape {Y.shape}: expected ({model.x.shape[0]}, Q) with Q >= 1")
    return Y


def targets_leaf_means(model, Y):
    """`mean[L, Q]`: for every leaf the mean of each column of `Y` over the leaf's own observations, `mean(Y[obs], axis=0)` --
    the ConstMean of a leaf built without a mean function (`src/treeStructure.jl:253`), column by column."""
    target = model.model if isinstance(model, GaussianProcess) else model
    Y = _targets_matrix(target, Y)
    return np.stack([np.mean(Y[lf.obs], axis=0) for lf in target.leaves])


def _targets_model(model, what):
    target = model.model if isinstance(model, GaussianProcess) else model
    if target.shard.world > 1:
        raise NotImplementedError(f"{what}: the model is sharded over several ranks; every rank solves its own leaves "
                                  "(Context.solve_targets), the exchange is out of scope")
    if not hasattr(_ctx_type(target), "solve_targets"):
        raise NotImplementedError(f"{what}: {_ctx_type(target).__name__} has no solve_targets")
    return target


def fit_targets(model, Y, mean=None):
    """Several target columns over the model's inputs on its CURRENT fit (no reference counterpart): `Y` is `(N, Q)`, one
    column per output -- joint torques, sensor channels, bootstrap or permuted targets.  Every leaf GP keeps its
    factorisation; the device solves `Z = L^-1 (Y[obs] - mean)` per leaf (`Context.solve_targets`: 2 n^2 flops per leaf and
    column instead of a refit's n^3 / 3).  Returns the `(L, Q)` table of log marginal likelihoods, `mll[l, j]` = that of leaf
    `l` with column `j` as its targets -- what a caller needs to re-weigh the sum nodes per column.
    Runs `fit(model)` first if the model has no fit.  `mean` is `(L, Q)`; `None` gives every leaf the mean of each column over
    its own observations (`targets_leaf_means`), the ConstMean of a leaf built without a mean function.  A `GaussianProcess`
    works too.  The model's own `y`, its fit and its weights are left as they are."""
    target = _targets_model(model, "fit_targets")
    Y = _targets_matrix(target, Y)
    mean = targets_leaf_means(target, Y) if mean is None else np.asarray(mean, dtype=np.float64).reshape(target.L, Y.shape[1])
    if not target._uploaded or np.all(np.isnan(target.leaf_mll)):
        fit(target)
    try:
        mll, sec = target.ctx.solve_targets(Y, mean)
    except hipabi.DsmgpError as e:
        if e.code != hipabi.E_STATE:
            raise
        fit(target)             # the hyper-parameters moved since the last fit
        mll, sec = target.ctx.solve_targets(Y, mean)
    target.last_targets_seconds = sec
    target.targets_mll = np.ascontiguousarray(mll)      # what targets_objective / grad_targets read
    target.targets_lpd = None                           # the LOO table of the columns belongs to the targets it was taken on
    return target.targets_mll.copy()


def _aggregate_host(model, xt, rc, mu, var):
    """`predict`'s aggregation of one set of per-(leaf, row) moments on the host, by the model's own rule."""
    if model.family == "dsmgp":
        if model.root.kind != "gp" and not model.tindex.weights_normalised():
            return _aggregate_dsmgp(model, xt, rc["ptr"], mu, var)      # the literal recursion with its mu_min - 1 shift
        return _aggregate_dsmgp_flat(model, xt.shape[0], rc, mu, var)
    return _aggregate_poe(model, xt, rc["ptr"], mu, var)


def _columns_device(model, target, what):
    """The context and the arguments of `Context.aggregate_columns` for `aggregate="device"`, after the refusals."""
    if target.family == "dsmgp" and target.root.kind != "gp" and not target.tindex.weights_normalised():
        raise ValueError(f"{what}: the sum weights are not normalised; the device aggregates the flat mixture only")
    if issubclass(_ctx_type(target), hipabi.StreamingContext):
        raise hipabi.DsmgpError(hipabi.E_STATE, f"{what}: a streaming context discards what the device aggregation reads")
    if not hasattr(_ctx_type(target), "aggregate_columns"):
        raise NotImplementedError(f"{what}: {_ctx_type(target).__name__} has no aggregate_columns (a single Context only)")
    family, coef, group, G, plain, prior = _aggregation_spec(target)
    return dict(family=family, leaf_coef=coef, leaf_group=group, n_groups=G, plain=plain, prior_kernel_id=prior.kernelid if prior else 0)


def predict_targets(model, xtest, aggregate="host"):
    """`(mu, var)`, both `(n_t, Q)`: `predict(model, xtest)` for every target column of the last `fit_targets` (no reference
    counterpart).  The per-(leaf, row) means of all columns come from the device (`Context.predict_targets`, on the `K_tn L^-T`
    of `predict`'s own sweep); the leaf variances do not depend on the targets.  The aggregation runs on the host, column by
    column, with the model's own rule (DSMGP mixture, PoE, gPoE, rBCM, single GP) and the clamps and the `mu_min - 1` shift
    rule of `predict`.  The sum-node weights are the ones the model holds -- those of its own `y`: this function does NOT
    re-weigh per column (the `mll` table of `fit_targets` is there for callers who want to).  The mixture variance depends on
    the column through `sum W mu^2 - mu^2`; the product-of-experts variances are the same in every column."""
    _check_aggregate("predict_targets", aggregate)
    target = _targets_model(model, "predict_targets")
    xt = _test_matrix(target, xtest)
    kw = _columns_device(model, target, "predict_targets") if aggregate == "device" else None
    Q = int(getattr(target.ctx, "targets_Q", 0))
    if Q < 1:
        raise hipabi.DsmgpError(hipabi.E_STATE, "predict_targets before fit_targets")
    n_t = xt.shape[0]
    if n_t == 0:
        return np.zeros((0, Q)), np.zeros((0, Q))
    if kw is not None:      # with `aggregate="device"`: the moments of every column in one call, nothing per entry is fetched
        predict(target, xt)         # routes, registers and runs as predict does
        mu, var = target.ctx.aggregate_columns(**kw)
        return np.ascontiguousarray(mu), np.ascontiguousarray(var)
    rc = _routing(target, xt)
    _, var_l = _leaf_moments(target, xt, rc)
    mu_l = target.ctx.predict_targets()
    mu = np.empty((n_t, Q))
    var = np.empty((n_t, Q))
    for j in range(Q):
        if isinstance(model, GaussianProcess):
            mu[:, j], var[:, j] = mu_l[:, j], np.where(var_l <= 0, EPS, var_l)
        else:
            mu[:, j], var[:, j] = _aggregate_host(target, xt, rc, np.ascontiguousarray(mu_l[:, j]), var_l)
    return mu, var


def predict_targets_gradients(model, xtest, aggregate="host"):
    """`(mu, var, dmu, dvar)`: `predict_targets(model, xtest)` -- `mu`, `var` of shape `(n_t, Q)` -- and the gradients of both
    moments with respect to the test point for every target column of the last `fit_targets`, `dmu`, `dvar` of shape
    `(n_t, Q, D)`: `dmu[t]` is the Jacobian of the vector-valued predictive mean at row t (no reference counterpart).  The
    per-(leaf, row) gradients of the means of all columns come from the device in one call (`Context.predict_targets_gradients`:
    a matrix product per dimension on the resident `A = K_y^-1 (Y - m)`), the leaf `dvar`, which does not depend on the targets,
    from `Context.predict_gradients`; the aggregation runs on the host, column by column (`aggregate_input_gradients`).  The
    mixture variance depends on the column through the means, so `dvar` differs per column for a DSMGP; it is the same in every
    column for PoE, gPoE, rBCM and a single GaussianProcess.  Refused: what `predict_gradients` and `predict_targets` refuse."""
    _check_aggregate("predict_targets_gradients", aggregate)
    target = _targets_model(model, "predict_targets_gradients")
    if target.family == "dsmgp" and target.root.kind != "gp" and not target.tindex.weights_normalised():
        raise ValueError("predict_targets_gradients: the sum weights are not normalised; predict then shifts the means by "
                         "mu_min - 1, which is not differentiable")
    if not hasattr(_ctx_type(target), "predict_targets_gradients"):
        raise NotImplementedError(f"predict_targets_gradients: {_ctx_type(target).__name__} has no predict_targets_gradients")
    if issubclass(_ctx_type(target), hipabi.StreamingContext):
        raise hipabi.DsmgpError(hipabi.E_STATE, "predict_targets_gradients: a streaming context discards what the input gradients read")
    xt = _test_matrix(target, xtest)
    n_t, D = xt.shape
    Q = int(getattr(target.ctx, "targets_Q", 0))
    if Q < 1:
        raise hipabi.DsmgpError(hipabi.E_STATE, "predict_targets_gradients before fit_targets")
    if n_t == 0:
        return np.zeros((0, Q)), np.zeros((0, Q)), np.zeros((0, Q, D)), np.zeros((0, Q, D))
    if aggregate == "device":               # (n_t, D, Q) from the device -> (n_t, Q, D); no per-entry array, no entry list
        kw = _columns_device(model, target, "predict_targets_gradients")
        mu, var = predict_targets(model, xt, aggregate="device")
        dmu, dvar = target.ctx.aggregate_columns_gradients(plain=kw["plain"], prior_kernel_id=kw["prior_kernel_id"])
        return mu, var, np.ascontiguousarray(dmu.transpose(0, 2, 1)), np.ascontiguousarray(dvar.transpose(0, 2, 1))
    mu, var = predict_targets(model, xt)    # routes, registers and runs as predict does; K_tn L^-T stays on the device
    rc = _routing(target, xt)
    ptr, idx = rc["lptr"], rc["lidx"]
    _, var_l = target.ctx.predict_fetch()
    mu_l = target.ctx.predict_targets()
    dmu_l = target.ctx.predict_targets_gradients()
    _, dvar_l = target.ctx.predict_gradients()
    dmu = np.empty((n_t, Q, D))
    dvar = np.empty((n_t, Q, D))
    if isinstance(model, GaussianProcess):
        for j in range(Q):
            dmu[:, j, :], dvar[:, j, :] = dmu_l[:, :, j], dvar_l
        return mu, var, dmu, dvar
    ent = [[] for _ in range(n_t)]
    for l in range(len(ptr) - 1):
        for k in range(int(ptr[l]), int(ptr[l + 1])):
            ent[int(idx[k])].append((l, k))
    family, coef, group, G, plain, prior = _aggregation_spec(target)
    kw = {}
    if family == hipabi.AGG_RBCM:
        kw = dict(kss_prior=_prior_diag(prior, xt), noise_prior=np.exp(2 * prior.logNoise), dkss_prior=_prior_diag_grad(prior, xt))
    for j in range(Q):
        dmu[:, j, :], dvar[:, j, :] = aggregate_input_gradients(family, np.ascontiguousarray(mu_l[:, j]), var_l,
                                                                np.ascontiguousarray(dmu_l[:, :, j]), dvar_l, ent, coef=coef,
                                                                group=group, G=G, plain=plain, **kw)
    return mu, var, dmu, dvar


def _ctx_type(model):
    """Type of the model's device context without creating it (a rank that owns no leaves never does)."""
    if model._ctx is not None:
        return type(model._ctx)
    if model._stream_budget is not None:
        return hipabi.StreamingContext
    return hipabi.MultiContext if model._n_sub > 1 else hipabi.Context


def _aggregation_spec(model):
    """(family, leaf_coef, leaf_group, n_groups, plain, prior_leaf) of `dsmgp_aggregate` for this model."""
    root = model.root
    if model.family == "dsmgp":
        return hipabi.AGG_MIXTURE, np.exp(model.tindex.leaf_path_logweights()), None, 0, root.kind == "gp", None
    if root.kind == "gp" or model.family == "poe":
        return hipabi.AGG_POE, np.ones(model.L), None, 0, False, None
    if model.family == "gpoe":
        return hipabi.AGG_GPOE, np.full(model.L, 1.0 / len(root.children)), None, 0, False, None      # src/common.jl:215
    group = np.zeros(model.L, dtype=np.int32)
    for g, c in enumerate(root.children):                                                                 # :231
        for lf in get_leaves(c):
            group[lf.leaf] = g
    return hipabi.AGG_RBCM, None, group, len(root.children), False, model.leaves[0]


def _finish_partial(model, xt, family, part, n_groups, plain, prior_leaf):
    """Host form of `agg_finish_kernel` on summed partial sums (several ranks or contexts hold the leaves)."""
    if family == hipabi.AGG_MIXTURE:
        m = part[0]
        return m, (part[2] if plain else part[2] + (part[1] - m * m))
    if family != hipabi.AGG_RBCM:
        return part[0] / part[1], 1.0 / part[1]
    s = _prior_diag(prior_leaf, xt) + np.exp(2 * prior_leaf.logNoise)
    Cc = 1.0 / s
    m = np.zeros(xt.shape[0])
    for g in range(n_groups):
        T = part[2 * g + 1]
        seen = T != 0.0                      # no leaf of this child saw the row: the group is skipped (agg_finish_kernel)
        Ts = np.where(seen, T, 1.0)
        M = part[2 * g] / Ts
        beta = 0.5 * (np.log(s) - np.log(1.0 / Ts))
        Cc = Cc + np.where(seen, (beta * Ts) - (beta / s), 0.0)
        m = m + np.where(seen, M * (beta * Ts), 0.0)
    return m / Cc, 1.0 / Cc


def _predict_device(model, xt, rc):
    family, coef, group, G, plain, prior = _aggregation_spec(model)
    loc = model.shard.local
    have = len(loc) > 0
    if have:
        _register_rows(model, xt, rc)
        model.last_predict_seconds = model.ctx.predict_run()
    single = model.shard.world == 1 and isinstance(model.ctx, hipabi.Context) and model.shard.comm_ctx is None
    if single:      # one context holds every leaf: partial sums, finish and (later) scores never leave the device
        mu, var = model.ctx.aggregate(family, coef, group, G, plain=plain, prior_kernel_id=prior.kernelid if prior else 0)
        model._scores_on_device = True
        return mu, var
    if model.shard.comm_ctx is not None:
        # the exchange step of predict inside the library: partial sums stay in HBM, are all-gathered over RCCL on the
        # context's stream and added in rank order on the device; the finish runs on the total
        W = hipabi.agg_width(family, G)
        if have:
            model.ctx.aggregate_partial(family, None if coef is None else coef[loc], None if group is None else group[loc], G,
                                        fetch=False)
            model.ctx.aggregate_exchange(W)
            mu, var = model.ctx.aggregate_finish(None, plain=plain, prior_kernel_id=prior.kernelid if prior else 0)
            model._scores_on_device = True
            return mu, var
        part = model.ctx.aggregate_exchange_empty(W, xt.shape[0])
        return _finish_partial(model, xt, family, part, G, plain, prior)
    if have:
        part = model.ctx.aggregate_partial(family, None if coef is None else coef[loc], None if group is None else group[loc], G)
    else:
        part = np.zeros((hipabi.agg_width(family, G), xt.shape[0]))
    part = model.shard.allgather_sum(part)          # the exchange step of predict: W x n_t doubles per rank
    return _finish_partial(model, xt, family, part, G, plain, prior)


def scores(model, y_test, mu=None, var=None):
    """dict(mse, sse, mae, sae, nlpd) (`src/scorefunctions.jl:6-16`) of the last `predict(model, x)`: computed on the
    device from the aggregated prediction still resident there when one context holds the model, else from (mu, var).
    A later `fit` drops the resident prediction (the context refuses `dsmgp_scores` on the sums of an earlier fit): call
    `predict` again, or pass the (mu, var) it returned."""
    y_test = np.ascontiguousarray(y_test, dtype=np.float64)
    if getattr(model, "_scores_on_device", False) and mu is None:
        return model.ctx.scores(y_test)
    if mu is None or var is None:
        raise ValueError("scores: pass the (mu, var) that predict returned (they are not resident on one device)")
    return dict(mse=mse(y_test, mu), sse=sse(y_test, mu), mae=mae(y_test, mu), sae=sae(y_test, mu), nlpd=nlpd(y_test, mu, var))


# ------------------------------------------------------------------------------------ leave-one-out

def loo(model):
    """Leave-one-out cross-validation of every leaf GP on the current fit (GPML 5.4.2, eqs. 5.10-5.12; `dsmgp_loo`), the mean
    and the hyper-parameters held fixed.  dict(obs, mu, var, lpd): per leaf, in the model's leaf order, `obs[l]` the leaf's
    training rows, `mu[l]` / `var[l]` the moments at those rows of the leaf's GP fitted without the row (`var` with noise and
    the fit's 1e-8 jitter), and `lpd[l]` the leaf's summed LOO log predictive density (an array of length L).  Works on a
    `GaussianProcess` too (one leaf).  Needs a fit.  Single rank only: with `shard.world > 1` it raises NotImplementedError
    (nothing is gathered)."""
    target = model.model if isinstance(model, GaussianProcess) else model
    if target.shard.world > 1:
        raise NotImplementedError("loo: leave-one-out moments are served on a single rank only")
    mu, var, lpd = target.ctx.loo()
    ptr, idx = obs_table(target.leaves)
    return dict(obs=[np.asarray(idx[ptr[l]:ptr[l + 1]], dtype=np.int64) for l in range(target.L)],
                mu=[mu[ptr[l]:ptr[l + 1]] for l in range(target.L)],
                var=[var[ptr[l]:ptr[l + 1]] for l in range(target.L)], lpd=lpd)


def _loo_substitute(ptr, idx, mu, var, obs, mu_loo, var_loo):
    """The per-(leaf, row) moments (CSR lists `ptr`, `idx` over the leaves; `mu`, `var` aligned with `idx`) with every entry
    whose row is one of its leaf's observations `obs[l]` replaced by that observation's leave-one-out moments
    (`mu_loo[l]`, `var_loo[l]`, aligned with `obs[l]`).  Entries of leaves that never saw the row are kept.  Returns copies."""
    mu = np.array(mu, dtype=np.float64)
    var = np.array(var, dtype=np.float64)
    for l in range(len(ptr) - 1):
        o = np.asarray(obs[l], dtype=np.int64)
        if o.size == 0 or ptr[l + 1] == ptr[l]:
            continue
        rows = np.asarray(idx[ptr[l]:ptr[l + 1]], dtype=np.int64)
        order = np.argsort(o, kind="stable")
        pos = np.minimum(np.searchsorted(o[order], rows), o.size - 1)
        hit = o[order][pos] == rows
        src = order[pos[hit]]
        mu[ptr[l]:ptr[l + 1]][hit] = np.asarray(mu_loo[l])[src]
        var[ptr[l]:ptr[l + 1]][hit] = np.asarray(var_loo[l])[src]
    return mu, var


def loo_predict(model):
    """(mu, var) per training row: `predict(model, model.x)` with, for every leaf that holds the row among its observations,
    that leaf's leave-one-out moments in place of its ordinary ones; leaves that never saw the row keep their prediction.
    The entries are aggregated by the model's own family rule on the host (the rules `predict` falls back to); tree weights
    and hyper-parameters stay as they are.  Single rank only (NotImplementedError with `shard.world > 1`, as `loo`)."""
    res = loo(model)
    if isinstance(model, GaussianProcess):
        model = model.model
    xt = model.x
    rc = _routing(model, xt)
    mu, var = _leaf_moments(model, xt, rc)
    mu, var = _loo_substitute(rc["ptr"], rc["idx"], mu, var, res["obs"], res["mu"], res["var"])
    if model.family == "dsmgp":
        if model.root.kind != "gp" and not model.tindex.weights_normalised():
            return _aggregate_dsmgp(model, xt, rc["ptr"], mu, var)
        return _aggregate_dsmgp_flat(model, xt.shape[0], rc, mu, var)
    return _aggregate_poe(model, xt, rc["ptr"], mu, var)


def loo_scores(model):
    """dict(mse, sse, mae, sae, nlpd) of the training targets against `loo_predict(model)`."""
    mu, var = loo_predict(model)
    y = (model.model if isinstance(model, GaussianProcess) else model).y
    return dict(mse=mse(y, mu), sse=sse(y, mu), mae=mae(y, mu), sae=sae(y, mu), nlpd=nlpd(y, mu, var))


# ------------------------------------------------------------------------------------ k-fold

def make_folds(n, K, seed=0, groups=None):
    """int32 fold labels 0 .. K - 1 for `n` rows, balanced (sizes differ by at most one) and shuffled with the portable counter
    stream of `datagen` (two machines draw the same folds).  With `groups` (one value per row) the units that are shuffled and
    dealt are the distinct groups, in the order of their first row: rows of one group share a label, and the labels are balanced
    in groups."""
    from .datagen import uniform
    n, K = int(n), int(K)
    if K < 1:
        raise ValueError("make_folds: K must be at least 1")
    if groups is None:
        unit = np.arange(n, dtype=np.int64)
        n_units = n
    else:
        groups = np.asarray(groups)
        if groups.shape != (n,):
            raise ValueError("make_folds: groups must have one value per row")
        _, first, inv = np.unique(groups, return_index=True, return_inverse=True)
        rank = np.empty(first.size, dtype=np.int64)
        rank[np.argsort(first, kind="stable")] = np.arange(first.size)     # groups numbered by their first row
        unit = rank[inv.reshape(-1)]
        n_units = first.size
    order = np.argsort(uniform(int(seed), 0, n_units), kind="stable")       # a permutation: unit order[j] is dealt j-th
    label = np.empty(n_units, dtype=np.int32)
    label[order] = (np.arange(n_units) % K).astype(np.int32)
    return np.ascontiguousarray(label[unit], dtype=np.int32)


def kfold(model, fold):
    """k-fold cross-validation of every leaf GP on the current fit (`dsmgp_kfold`; the multiple-fold residual formulas), the
    mean and the hyper-parameters held fixed: `fold[r]` is the label of training row r, -1 (never held out) .. K - 1 with
    K = max(fold) + 1.  dict(obs, mu, var, lpd, info) per leaf in the model's leaf order, in the shape of `loo(model)`:
    `mu[l]` / `var[l]` the moments at the leaf's rows of the leaf's GP fitted without the rows that share the row's label (NaN
    for label -1), `lpd` `(L, K)` the joint log predictive density of every (leaf, label) block and `info` `(L, K)` its flag.
    Works on a `GaussianProcess` too.  Single rank only, as `loo`."""
    target = model.model if isinstance(model, GaussianProcess) else model
    if target.shard.world > 1:
        raise NotImplementedError("kfold: k-fold moments are served on a single rank only")
    fold = np.ascontiguousarray(fold, dtype=np.int32)
    if fold.shape != (target.x.shape[0],):
        raise ValueError("kfold: fold must have one label per training row")
    mu, var, lpd, info = target.ctx.kfold(fold)
    ptr, idx = obs_table(target.leaves)
    return dict(obs=[np.asarray(idx[ptr[l]:ptr[l + 1]], dtype=np.int64) for l in range(target.L)],
                mu=[mu[ptr[l]:ptr[l + 1]] for l in range(target.L)],
                var=[var[ptr[l]:ptr[l + 1]] for l in range(target.L)], lpd=np.asarray(lpd), info=np.asarray(info))


def _kfold_held(obs, mu, var, fold):
    """The per-leaf tables of `kfold` without the rows that are never held out (label -1): what `_loo_substitute` takes."""
    keep = [np.asarray(fold)[np.asarray(o, dtype=np.int64)] >= 0 for o in obs]
    return ([np.asarray(o)[k] for o, k in zip(obs, keep)], [np.asarray(m)[k] for m, k in zip(mu, keep)],
            [np.asarray(v)[k] for v, k in zip(var, keep)])


def kfold_predict(model, fold):
    """(mu, var) per training row: `loo_predict`'s construction with the held-out moments of `kfold(model, fold)` substituted --
    for every leaf that holds the row among its observations, that leaf's moments fitted without the row's fold; leaves that
    never saw the row, and rows with label -1, keep their ordinary prediction.  The entries are aggregated by the model's own
    family rule on the host.  Single rank only."""
    res = kfold(model, fold)
    if isinstance(model, GaussianProcess):
        model = model.model
    xt = model.x
    rc = _routing(model, xt)
    mu, var = _leaf_moments(model, xt, rc)
    obs, mu_k, var_k = _kfold_held(res["obs"], res["mu"], res["var"], fold)
    mu, var = _loo_substitute(rc["ptr"], rc["idx"], mu, var, obs, mu_k, var_k)
    if model.family == "dsmgp":
        if model.root.kind != "gp" and not model.tindex.weights_normalised():
            return _aggregate_dsmgp(model, xt, rc["ptr"], mu, var)
        return _aggregate_dsmgp_flat(model, xt.shape[0], rc, mu, var)
    return _aggregate_poe(model, xt, rc["ptr"], mu, var)


def kfold_scores(model, fold):
    """dict(mse, sse, mae, sae, nlpd) of the training targets against `kfold_predict(model, fold)`, over the rows that were
    held out (label >= 0)."""
    mu, var = kfold_predict(model, fold)
    y = (model.model if isinstance(model, GaussianProcess) else model).y
    held = np.asarray(fold) >= 0
    y, mu, var = y[held], mu[held], var[held]
    return dict(mse=mse(y, mu), sse=sse(y, mu), mae=mae(y, mu), sae=sae(y, mu), nlpd=nlpd(y, mu, var))


def _aggregate_dsmgp_flat(model, n_t, rc, mu, var):
    """The nested log-domain recursion of `_predict` (`src/common.jl:275-302`) is linear in the leaf quantities
    (mu - c, mu^2, sigma^2): unrolled, a test row's prediction is the flat mixture over the leaves it visits with
    weight = product of the sum-node weights on the leaf's path (split nodes only route).  So
        mu = sum_l W_l mu_l,   v = sum_l W_l sigma2_l + sum_l W_l mu_l^2 - mu^2
    in three weighted bincounts over the (leaf, row) entries.  `_aggregate_dsmgp` below is the literal recursion,
    kept as the cross-check (tests/test_host_cpu.py)."""
    logW = model.tindex.leaf_path_logweights()
    ptr, idx = rc["ptr"], rc["idx"]
    w = np.repeat(np.exp(logW), np.diff(ptr))
    s2 = np.where(var <= 0, EPS, var)                       # src/common.jl:137
    m = np.bincount(idx, weights=w * mu, minlength=n_t)
    m2 = np.bincount(idx, weights=w * mu * mu, minlength=n_t)
    sv = np.bincount(idx, weights=w * s2, minlength=n_t)
    if model.root.kind == "gp":
        return m, sv
    return m, sv + (m2 - m * m)


def _aggregate_dsmgp(model, xt, ptr, mu, var, sel_cache=None):
    """Sum/product aggregation of the leaf moments exactly as `_minpredict` + `_predict`
    (`src/common.jl:134-196,275-302`) do it, from ONE set of leaf predictions."""
    n_t = xt.shape[0]
    all_rows = np.arange(n_t, dtype=np.int64)
    sel_cache = {} if sel_cache is None else sel_cache

    def child_masks(node, rows):
        """getchild once per split node: the three recursions below partition the rows identically."""
        m = sel_cache.get(node.id)
        if m is None:
            ch = get_child(node, xt[rows])
            m = sel_cache[node.id] = [ch == k for k in range(len(node.children))]
        return m

    def leaf_vals(node):
        a, b = ptr[node.leaf], ptr[node.leaf + 1]
        return mu[a:b], var[a:b]

    def minpred(node, rows):
        if node.kind == "gp":
            return leaf_vals(node)[0]
        if node.kind == "split":
            out = np.zeros(rows.size)
            for sel, c in zip(child_masks(node, rows), node.children):
                out[sel] = minpred(c, rows[sel])
            return out
        out = np.full(rows.size, np.inf)
        for c in node.children:
            out = np.minimum(out, minpred(c, rows))
        return out

    def pred(node, rows, mmin):
        if node.kind == "gp":
            m, s2 = leaf_vals(node)
            s2 = np.where(s2 <= 0, EPS, s2)  # src/common.jl:137
            if not np.all(m >= mmin):
                raise AssertionError("leaf mean below the shift (src/common.jl:138)")
            with np.errstate(divide="ignore"):
                return np.log(m - mmin), np.log(m * m), np.log(s2)
        if node.kind == "split":
            lm = np.zeros(rows.size)
            lm2 = np.zeros(rows.size)
            ls = np.zeros(rows.size)
            for sel, c in zip(child_masks(node, rows), node.children):
                a, b, d = pred(c, rows[sel], mmin[sel])
                lm[sel], lm2[sel], ls[sel] = a, b, d
            return lm, lm2, ls
        K = len(node.children)
        lm = np.zeros((rows.size, K))
        lm2 = np.zeros((rows.size, K))
        ls = np.zeros((rows.size, K))
        for k, c in enumerate(node.children):
            a, b, d = pred(c, rows, mmin)
            lm[:, k] = a + node.logweights[k]
            lm2[:, k] = b + node.logweights[k]
            ls[:, k] = d + node.logweights[k]
        return _logsumexp(lm, axis=1), _logsumexp(lm2, axis=1), _logsumexp(ls, axis=1)

    def predict_node(node, rows):
        if node.kind == "gp":                    # src/common.jl:175-179
            m, s2 = leaf_vals(node)
            return m, np.where(s2 <= 0, EPS, s2)
        if node.kind == "split":                 # src/common.jl:243-254
            m = np.zeros(rows.size)
            v = np.zeros(rows.size)
            for sel, c in zip(child_masks(node, rows), node.children):
                m[sel], v[sel] = predict_node(c, rows[sel])
            return m, v
        mmin = minpred(node, rows)               # src/common.jl:294-302
        lm, lm2, ls = pred(node, rows, mmin - 1.0)
        m = np.exp(lm) + mmin - 1.0
        return m, np.exp(ls) + (np.exp(lm2) - m * m)

    return predict_node(model.root, all_rows)


def _prior_diag(lf, xt):
    k = lf.kernel
    if k.kind in (KIND_ISO_SE, KIND_ARD_SE_PRODUCT, KIND_ISO_MATERN32, KIND_ISO_MATERN52, KIND_ARD_MATERN32, KIND_ARD_MATERN52,
                  KIND_ISO_RQ, KIND_ARD_RQ):
        return np.full(xt.shape[0], np.exp(2 * k.logs))
    if k.kind == KIND_ARD_SE:
        return np.full(xt.shape[0], np.exp(2 * k.logs) * xt.shape[1])
    if k.kind == KIND_ARD_LINEAR:
        return (xt * xt) @ np.exp(-2.0 * k.logl)
    return np.sum(xt * xt, axis=1) / np.exp(k.logl) ** 2


def _aggregate_poe(model, xt, ptr, mu, var):
    """PoE / gPoE / rBCM combination rules (`src/common.jl:145-149,198-273`)."""
    n_t = xt.shape[0]

    def poe(node):
        if node.kind == "gp":
            a, b = ptr[node.leaf], ptr[node.leaf + 1]
            return mu[a:b], 1.0 / var[a:b]
        m = np.zeros(n_t)
        t = np.zeros(n_t)
        for c in node.children:
            m_, t_ = poe(c)
            t += t_
            m += t_ * m_
        return m / t, t

    root = model.root
    if root.kind == "gp":
        m, t = poe(root)
        return m, 1.0 / t
    if model.family == "poe":
        m, t = poe(root)
        return m, 1.0 / t
    if model.family == "gpoe":
        beta = 1.0 / len(root.children)
        m = np.zeros(n_t)
        t = np.zeros(n_t)
        for c in root.children:
            m_, t_ = poe(c)
            t += beta * t_
            m += beta * t_ * m_
        return m / t, 1.0 / t
    lf0 = get_leaves(root)[0]
    s = _prior_diag(lf0, xt) + np.exp(2 * lf0.logNoise)
    Cc = 1.0 / s
    m = np.zeros(n_t)
    for c in root.children:
        m_, t_ = poe(c)
        s_ = 1.0 / t_
        beta = 0.5 * (np.log(s) - np.log(s_))
        Cc = Cc + (beta * t_) - (beta / s)
        m = m + m_ * (beta * t_)
    return m / Cc, 1.0 / Cc


# ------------------------------------------------------------------------------------ scores

def mse(y_true, y_pred):
    return float(np.mean((np.asarray(y_true) - np.asarray(y_pred)) ** 2))


def mae(y_true, y_pred):
    return float(np.mean(np.abs(np.asarray(y_true) - np.asarray(y_pred))))


def sse(y_true, y_pred):
    """standard error of the squared error (`src/scorefunctions.jl:9`; Julia's std is the unbiased one)."""
    se = (np.asarray(y_true) - np.asarray(y_pred)) ** 2
    return float(np.std(se, ddof=1) / np.sqrt(se.size))


def sae(y_true, y_pred):
    """`src/scorefunctions.jl:14`"""
    ae = np.abs(np.asarray(y_true) - np.asarray(y_pred))
    return float(np.std(ae, ddof=1) / np.sqrt(ae.size))


def nlpd(y_true, mu, var):
    """`src/scorefunctions.jl:16`."""
    y_true, mu, var = map(np.asarray, (y_true, mu, var))
    return float(np.mean(0.5 * np.log(2 * np.pi * var) + 0.5 * (y_true - mu) ** 2 / var))
