"""GPU tests of dsmgp_loo: leave-one-out moments of every leaf GP (GPML 5.4.2, eqs. 5.10-5.12) from the diagonal of K_y^-1
(rownorm_kernel over L^-T) and alpha (loo_moments_kernel), through hipabi.Context.loo and the model API.

References: tests/golden/gp_loo.npz (50 digits, tests/golden/make_loo_golden.py) for single leaves; for leaf tables, the larger
single GP and the models a float64 reference formed in the test by tests/loo_dense.py from download_factor / kernel_matrix of
the same context -- twice the tolerance there, both sides round.  Tolerances: loo_dense.loo_tol (pred_tolerance.moment_tol for
the moments, carried through the density for lpd)."""
import math
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_kernels as dk
import loo_dense
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel
from pred_tolerance import agg_tol, aggregate, moment_tol, row_entries, score_tol

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = loo_dense.load_cases()
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}
GRAD = np.load(os.path.join(GOLDEN, "gp_grad.npz"))
SRC, CPY, PRE = 0, 32, 26       # the table's COPY leaf (of leaf 0) and its PREFIX leaf (of leaf 2)


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def lib_noise(logNoise):
    return math.exp(2.0 * float(logNoise))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _check(tag, got, ref, tol):
    """Every element within its tolerance; prints the worst error and error / tolerance."""
    got, ref, tol = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, ref, tol))
    err = np.abs(got - ref)
    ratio = err / tol
    worst = int(np.argmax(ratio)) if ratio.size else 0
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    assert np.all(err <= tol), (tag, worst, got.flat[worst], ref.flat[worst], tol.flat[worst])
    return float(np.max(ratio))


def _single(ctx, X, y, mean, kind, loghyp, logNoise):
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(mean)])
    ctx.set_hyper(0, int(kind), np.concatenate([loghyp, [float(logNoise)]]))
    _, info, _ = ctx.fit()
    assert info[0] == 0


def _lpd_of(y, mu, var):
    return loo_dense.lpd_terms(np.asarray(y, dtype=np.float64), mu, var)


# ------------------------------------------------------------------------------------- (1) fixture cases

@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_against_50_digit_references(ctx, name):
    c = CASES[name]
    _single(ctx, c["X"], c["y"], c["mean"], c["kind"], c["loghyp"], c["logNoise"])
    mu, var, lpd = ctx.loo()
    n = c["y"].size
    assert mu.shape == (n,) and var.shape == (n,) and lpd.shape == (1,)
    tm, tv, tl, ts = loo_dense.loo_tol(c["y"], c["mu"], c["var"], c["kss"], lib_noise(c["logNoise"]))
    _check(name + " mu", mu, c["mu"], tm)
    _check(name + " var", var, c["var"], tv)
    _check(name + " lpd_i from the moments", _lpd_of(c["y"], mu, var), c["lpd"], tl)
    _check(name + " lpd", lpd[0], c["lpd_sum"], ts)
    mu2, var2, lpd2 = ctx.loo()
    assert _same_bits(mu, mu2) and _same_bits(var, var2) and _same_bits(lpd, lpd2)


# ------------------------------------------------------------------------------------- (2) leaf tables, a large single GP

def _table_setup(ctx, mean=None):
    T = TABLE
    ctx.set_train(T["X"], T["y"])
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean"] if mean is None else mean)
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])


def _table_check(ctx, tag, mean, got, factor=2.0):
    """Every leaf of the table against the dense helper on its downloaded factor; returns the worst err / tol."""
    T = TABLE
    op_, ob = T["obs_ptr"], T["obs_idx"]
    mu, var, lpd = got
    worst = 0.0
    for l in range(T["kid"].size):
        a, b = int(op_[l]), int(op_[l + 1])
        rows = ob[a:b]
        kid = int(T["kid"][l])
        noise = lib_noise(T["hyp"][kid][T["hyp_len"][kid] - 1])
        F, _ = ctx.download_factor(l, b - a)
        yl = T["y"][rows]
        rm, rv, rl = loo_dense.loo_from_factor(F, yl, float(mean[l]))
        Xl = np.asfortranarray(T["X"][rows])
        kss = np.diag(ctx.kernel_matrix(kid, Xl, Xl))
        tm, tv, tl, ts = loo_dense.loo_tol(yl, rm, rv, kss, noise)
        r = [np.max(np.abs(mu[a:b] - rm) / (factor * tm)), np.max(np.abs(var[a:b] - rv) / (factor * tv)),
             abs(lpd[l] - np.sum(rl)) / (factor * ts)]
        assert max(r) <= 1.0, (tag, l, r)
        worst = max(worst, float(max(r)))
    print(f"\n{tag}: {T['kid'].size} leaves, worst err/tol {worst:.3g}")
    return worst


def test_leaf_table_with_copy_and_prefix_leaves(ctx):
    """The 41-leaf table of gp_pred.npz (FULL leaves of four kernel ids, a COPY and a PREFIX leaf), the COPY leaf once with its
    source's mean and once with another: every leaf against the dense helper on download_factor of the same context."""
    T = TABLE
    assert T["op"][CPY] == 1 and T["src"][CPY] == SRC and T["op"][PRE] == 2 and T["mean"][CPY] == T["mean"][SRC]
    a, b = (int(v) for v in T["obs_ptr"][CPY:CPY + 2])
    s0, s1 = (int(v) for v in T["obs_ptr"][SRC:SRC + 2])
    _table_setup(ctx)
    _, info, _ = ctx.fit()
    assert np.all(info == 0)
    same = ctx.loo()
    _table_check(ctx, "table, COPY leaf with its source's mean", T["mean"], same)
    assert _same_bits(same[0][a:b], same[0][s0:s1]) and _same_bits(same[1][a:b], same[1][s0:s1])
    assert _same_bits(same[2][CPY], same[2][SRC])
    mean2 = T["mean"].copy()
    mean2[CPY] += 0.37
    _table_setup(ctx, mean2)
    _, info, _ = ctx.fit()
    assert np.all(info == 0)
    other = ctx.loo()
    _table_check(ctx, "table, COPY leaf with another mean", mean2, other)
    assert _same_bits(other[1][a:b], same[1][a:b])                  # the variances do not see the mean
    assert not _same_bits(other[0][a:b], same[0][a:b])
    keep = np.ones(same[0].size, dtype=bool)
    keep[a:b] = False
    assert _same_bits(other[0][keep], same[0][keep]) and _same_bits(other[1][keep], same[1][keep])


def test_single_gp_n4096(ctx):
    """One leaf with 32 row tiles: 272 row-sum tasks, up to 16 slices per row."""
    n, D = 4096, 8
    X, y, _ = dsm.regression_data(n, D, n_test=8, seed=4096)
    hyp = np.array([np.log(0.9), 0.0])
    logNoise = np.log(0.1)
    mean = float(np.mean(y))
    _single(ctx, X, y, mean, 0, hyp, logNoise)
    mu, var, lpd = ctx.loo()
    t_alone = ctx.loo_seconds
    F, _ = ctx.download_factor(0, n)
    rm, rv, rl = loo_dense.loo_from_factor(F, y, mean)
    tm, tv, tl, ts = loo_dense.loo_tol(y, rm, rv, np.full(n, 1.0), lib_noise(logNoise))
    _check("n4096 mu", mu, rm, 2.0 * tm)
    _check("n4096 var", var, rv, 2.0 * tv)
    _check("n4096 lpd", lpd[0], np.sum(rl), 2.0 * ts)
    again = ctx.loo()
    assert _same_bits(mu, again[0]) and _same_bits(var, again[1]) and _same_bits(lpd, again[2])
    print(f"loo device seconds: {t_alone:.3g} with the inversion, {ctx.loo_seconds:.3g} reusing it")


# ------------------------------------------------------------------------------------- (3) on bits

def test_reuse_mask_and_gradients_on_bits(ctx):
    """loo() after gradients() equals loo() alone; a gradient mask does not change it; gradients() after loo() equals
    gradients() alone, with and without a mask: under a mask loo() inverts the owners it left out over lists of its own and
    drops them, so the masked pass runs the same launches before and after."""
    T = TABLE
    L = T["kid"].size
    stride = int(np.max(T["hyp_len"]))
    _table_setup(ctx)
    ctx.fit()
    alone = ctx.loo()
    ctx.fit()
    g_alone = ctx.gradients(stride)
    after = ctx.loo()                                   # reuses the inverse of the gradient pass
    assert all(_same_bits(p, q) for p, q in zip(alone, after))
    ctx.fit()
    first = ctx.loo()
    g_after = ctx.gradients(stride)
    assert all(_same_bits(p, q) for p, q in zip(alone, first)) and _same_bits(g_alone, g_after)
    mask = np.zeros(L, dtype=np.int32)
    mask[[3, 7, CPY]] = 1
    try:
        ctx.set_gradient_leaves(mask)
        ctx.fit()
        g_mask = ctx.gradients(stride)                  # lists without the owners the mask leaves out
        masked = ctx.loo()                              # ... which are built on demand
        assert all(_same_bits(p, q) for p, q in zip(alone, masked))
        g_mask2 = ctx.gradients(stride)                 # the mask's lists again: the same launches, the same bits
        assert _same_bits(g_mask, g_mask2)
        assert np.all(g_mask[mask == 0] == 0.0) and np.all(np.isfinite(g_mask[mask != 0]))
        assert all(_same_bits(p, q) for p, q in zip(alone, ctx.loo()))     # after a masked pass rewrote some owners
        ctx.fit()
        assert all(_same_bits(p, q) for p, q in zip(alone, ctx.loo()))     # loo() first under the mask
        assert all(_same_bits(p, q) for p, q in zip(alone, ctx.loo()))     # ... and again, reusing its own inverse
        assert _same_bits(g_mask, ctx.gradients(stride))
    finally:
        ctx.set_gradient_leaves(None)
    assert _same_bits(g_alone, ctx.gradients(stride))


@pytest.mark.parametrize("name", ["isose_n129", "ardse_d3", "ardlinear_d5"])
def test_gradients_unchanged_around_loo(ctx, name):
    """Cases of tests/golden/gp_grad.npz: the gradient of a fit is the same to the bit before and after loo() on that fit."""
    X, y = GRAD[f"{name}/X"], GRAD[f"{name}/y"]
    loghyp = GRAD[f"{name}/loghyp"]
    _single(ctx, X, y, float(GRAD[f"{name}/mean"]), int(GRAD[f"{name}/kind"]), loghyp, float(GRAD[f"{name}/logNoise"]))
    g0 = ctx.gradients(loghyp.size + 1)
    ctx.loo()
    g1 = ctx.gradients(loghyp.size + 1)
    ctx.fit()
    ctx.loo()
    g2 = ctx.gradients(loghyp.size + 1)
    assert _same_bits(g0, g1) and _same_bits(g0, g2)
    ref = GRAD[f"{name}/grad"]
    print(f"\n{name}: max |grad - 50 digits| {np.max(np.abs(g0[0, :ref.size] - ref)):.3g}")


def test_multicontext_puts_the_leaves_back_in_table_order(ctx):
    """Two sub-contexts share the 41-leaf table (sharing groups together): every leaf of MultiContext.loo, back in the order of
    the whole table, against the dense helper on the single context's factors, and against Context.loo within the tolerance
    both carry (not on bits: how a launch of the inversion is cut along K depends on the leaves it holds)."""
    T = TABLE
    _table_setup(ctx)
    _, info, _ = ctx.fit()
    assert np.all(info == 0)
    one = ctx.loo()
    mc = hipabi.MultiContext(0, 2)
    try:
        _table_setup(mc)
        _, info, _ = mc.fit()
        assert np.all(info == 0) and len(mc.act) == 2
        two = mc.loo()
        assert mc.loo_seconds > 0.0
    finally:
        mc.close()
    assert all(p.shape == q.shape for p, q in zip(one, two))
    _table_check(ctx, "table, two sub-contexts", T["mean"], two)
    print(f"same bits as one context: {[_same_bits(p, q) for p, q in zip(one, two)]}")


# ------------------------------------------------------------------------------------- (4) lanes, fused steps

def test_lanes_and_step_kinds_agree(ctx):
    T = TABLE
    got = {}
    try:
        for lanes, fused in ((1, 1), (2, 1), (1, 0), (2, 0)):
            ctx.set_option(hipabi.OPT_FUSED_STEPS, fused)
            ctx.set_option(hipabi.OPT_LANES, lanes)
            _table_setup(ctx)
            _, info, _ = ctx.fit()
            assert np.all(info == 0) and ctx.lanes() == lanes
            got[(lanes, fused)] = ctx.loo()
            _table_check(ctx, f"table lanes={lanes} fused_steps={fused}", T["mean"], got[(lanes, fused)])
        assert all(_same_bits(p, q) for p, q in zip(got[(1, 1)], got[(2, 1)]))      # per-leaf results do not depend on the lane
        assert all(_same_bits(p, q) for p, q in zip(got[(1, 0)], got[(2, 0)]))
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)


# ------------------------------------------------------------------------------------- (5) the model API

def _build(family, X, y):
    kern = dsm.IsoSE(np.log(0.3), 0.0)
    if family == "dsmgp":
        return dsm.buildDSMGP(X, y, 2, 3, M=40, kernel=kern, logNoise=np.log(0.1), seed=1)
    if family == "poe":
        return dsm.buildPoE(X, y, 3, M=40, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), logNoise=np.log(0.1), seed=1)
    return dsm.buildBCM(X, y, 3, M=40, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), logNoise=np.log(0.1), seed=1)


@pytest.mark.parametrize("family", ["dsmgp", "poe", "rbcm"])
def test_model_loo_predict_and_scores(family):
    """loo_predict against the same substitution done here with dense LOO moments (from the downloaded factors) and the
    aggregation formula of pred_tolerance.aggregate, tolerances carried through agg_tol; loo_scores through score_tol."""
    X, y, _ = dsm.regression_data(420, 2, n_test=8, seed=99)
    model = _build(family, X, y)
    try:
        n, L = X.shape[0], model.L
        res = dsm.loo(model)
        noise = lib_noise(model.leaves[0].logNoise)
        kss1 = math.exp(2.0 * model.leaves[0].kernel.logs)
        yscale = max(1.0, float(np.max(np.abs(y))))
        rc = dmodel._routing(model, model.x)
        mu_e, var_e = dmodel._leaf_moments(model, model.x, rc)
        ptr, idx = rc["ptr"], rc["idx"]
        tm_e, tv_e = moment_tol(mu_e, var_e, np.full(mu_e.size, kss1), noise, yscale)
        ref_mu, ref_var = mu_e.copy(), var_e.copy()
        nsub = 0
        for l, lf in enumerate(model.leaves):
            obs = np.asarray(lf.obs, dtype=np.int64)
            assert np.array_equal(res["obs"][l], obs)
            F, _ = model.ctx.download_factor(l, obs.size)
            rm, rv, rl = loo_dense.loo_from_factor(F, y[obs], lf.mean.m)
            tm, tv, _, ts = loo_dense.loo_tol(y[obs], rm, rv, np.full(obs.size, kss1), noise)
            assert np.all(np.abs(res["mu"][l] - rm) <= 2.0 * tm) and np.all(np.abs(res["var"][l] - rv) <= 2.0 * tv)
            assert abs(res["lpd"][l] - np.sum(rl)) <= 2.0 * ts
            where = {int(r): i for i, r in enumerate(obs)}
            for e in range(int(ptr[l]), int(ptr[l + 1])):
                i = where.get(int(idx[e]))
                if i is not None:
                    ref_mu[e], ref_var[e], tm_e[e], tv_e[e] = rm[i], rv[i], 2.0 * tm[i], 2.0 * tv[i]
                    nsub += 1
        assert 0 < nsub <= sum(o.size for o in res["obs"])      # (an observation in a leaf's overlap zone is not routed to it)
        fam, coef, group, G, plain, prior = dmodel._aggregation_spec(model)
        ent = row_entries(ptr, idx, n)
        kw = dict(coef=coef, group=group, G=G, plain=plain)
        if fam == hipabi.AGG_RBCM:
            kw.update(kss_prior=np.full(n, kss1), noise_prior=noise)
        am, av = aggregate(fam, list(ref_mu), list(ref_var), ent, log=math.log, **kw)
        am, av = np.array(am, dtype=np.float64), np.array(av, dtype=np.float64)
        S1 = None
        if fam == hipabi.AGG_MIXTURE:
            S1 = np.array([sum(float(coef[l]) * ref_mu[e] ** 2 for l, e in er) for er in ent])
        tm, tv = agg_tol(fam, ref_mu, ref_var, tm_e, tv_e, ent, S1=S1, **kw)
        mu, var = dsm.loo_predict(model)
        _check(f"{family} loo_predict mu", mu, am, tm)
        _check(f"{family} loo_predict var", var, av, tv)
        plain_mu, _ = dsm.predict(model, model.x)
        assert np.max(np.abs(plain_mu - mu)) > 1e-6              # held-out predictions are not the in-sample ones
        sc = dsm.loo_scores(model)
        ref_sc = [dsm.mse(y, am), dsm.sse(y, am), dsm.mae(y, am), dsm.sae(y, am), dsm.nlpd(y, am, av)]
        _check(f"{family} loo_scores", [sc[k] for k in hipabi.SCORE_NAMES], ref_sc, score_tol(y, am, av, tm, tv))
    finally:
        model.ctx.close()


def test_model_loo_on_a_gaussian_process():
    c = CASES["ardse_n128"]
    kern = dsm.ArdSE(c["loghyp"][:-1], float(c["loghyp"][-1]))
    gp = dsm.GaussianProcess(c["X"], c["y"], mean=dsm.ConstMean(c["mean"]), kernel=kern, logNoise=c["logNoise"], run_cholesky=True)
    try:
        res = dsm.loo(gp)
        tm, tv, _, ts = loo_dense.loo_tol(c["y"], c["mu"], c["var"], c["kss"], lib_noise(c["logNoise"]))
        assert np.array_equal(res["obs"][0], np.arange(c["y"].size))
        _check("gp loo mu", res["mu"][0], c["mu"], tm)
        _check("gp loo var", res["var"][0], c["var"], tv)
        _check("gp loo lpd", res["lpd"][0], c["lpd_sum"], ts)
        mu, var = dsm.loo_predict(gp)                   # one leaf, every row its own: the LOO moments themselves
        assert _same_bits(mu, res["mu"][0]) and _same_bits(var, res["var"][0])
    finally:
        gp.model.ctx.close()


# ------------------------------------------------------------------------------------- (6) arguments, state, failed leaves

def test_errors_and_null_outputs():
    c = CASES["isose_n127"]
    n = c["y"].size
    ctx = hipabi.Context(0)
    try:
        lib, dp = ctx.lib, hipabi._dp
        assert lib.dsmgp_loo(None, None, None, None, None) == hipabi.E_ARG
        ctx.set_train(c["X"], c["y"])
        ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
        ctx.set_hyper(0, c["kind"], np.concatenate([c["loghyp"], [c["logNoise"]]]))
        with pytest.raises(hipabi.DsmgpError) as e:         # before fit
            ctx.loo()
        assert e.value.code == hipabi.E_STATE
        ctx.fit()
        mu, var, lpd = ctx.loo()
        assert lib.dsmgp_loo(ctx.h, None, None, None, None) == 0          # every output may be NULL
        m2, v2, l2 = np.empty(n), np.empty(n), np.empty(1)
        assert lib.dsmgp_loo(ctx.h, m2.ctypes.data_as(dp), None, None, None) == 0
        assert lib.dsmgp_loo(ctx.h, None, v2.ctypes.data_as(dp), None, None) == 0
        assert lib.dsmgp_loo(ctx.h, None, None, l2.ctypes.data_as(dp), None) == 0
        assert _same_bits(mu, m2) and _same_bits(var, v2) and _same_bits(lpd, l2)
        ctx.set_hyper(0, c["kind"], np.concatenate([c["loghyp"] + 0.1, [c["logNoise"]]]))
        with pytest.raises(hipabi.DsmgpError) as e:         # new hyper-parameters: no fit yet
            ctx.loo()
        assert e.value.code == hipabi.E_STATE
        ctx.fit()
        assert not _same_bits(mu, ctx.loo()[0])
        ctx.release()
        with pytest.raises(hipabi.DsmgpError) as e:         # after release
            ctx.loo()
        assert e.value.code == hipabi.E_STATE
    finally:
        ctx.close()


def test_failed_leaf_gets_nan_and_the_others_are_unaffected(ctx):
    """Leaf 0: a rank-1 linear Gram of size 1e16 (not positive definite in float64, as test_not_positive_definite_is_reported);
    leaf 1: an ordinary IsoSE leaf."""
    n0, n1 = 140, 100
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    hyp1 = np.array([np.log(0.3), 0.0])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, np.concatenate([hyp1, [np.log(0.1)]]))
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    mu, var, lpd = ctx.loo()
    assert np.all(np.isnan(mu[:n0])) and np.all(np.isnan(var[:n0])) and np.isnan(lpd[0])
    K = dk.value(0, hyp1, X[n0:], X[n0:])
    rm, rv, rl = loo_dense.loo_dense(K, lib_noise(np.log(0.1)), y[n0:], 0.2)
    tm, tv, _, ts = loo_dense.loo_tol(y[n0:], rm, rv, np.diag(K), lib_noise(np.log(0.1)))
    _check("good leaf mu", mu[n0:], rm, 2.0 * tm)
    _check("good leaf var", var[n0:], rv, 2.0 * tv)
    _check("good leaf lpd", lpd[1], np.sum(rl), 2.0 * ts)
