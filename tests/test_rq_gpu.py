"""GPU suite for the rational quadratic kernels (DSMGP kinds 9 and 10): Gram tiles, single leaves, log-marginal and LOO gradients
(the shape's da included), input gradients and the predictive covariance against the dense restatement of tests/dense_gp.py,
the iso kind as the ARD kind with equal length-scales (bit for bit), gradients by central differences of the device's own
log-marginal and LOO density at D up to 48 with duplicate training points, COPY / PREFIX leaves and masks, all eleven kinds in
one context, a pooled context, whole models, a mixed kernel vector, train! and the refusals.  Tolerances come from
tests/pred_tolerance.py (mll_tol, moment_tol), tests/loo_dense.py, tests/predgrad_dense.py and the gradient rule
64 cond_2(K_y) eps max(1, |g|_inf) of tests/test_gradients_gpu.py; every group prints its worst err/tol."""
import itertools

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi, tree as ptree
from deepstructuredmixtures_amd.datagen import uniform, normal, regression_data
from oracle import spn as ospn
import dense_kernels as dk
from dense_gp import DenseGP
from test_rq_host import KINDS, ISO_RQ, ARD_RQ, is_ard, load_cases
from pred_tolerance import EPS, mll_tol, moment_tol
from loo_dense import loo_tol
import predgrad_dense as pgd

pytestmark = pytest.mark.gpu

WORST = {}
CLASSES = {ISO_RQ: dsm.IsoRQ, ARD_RQ: dsm.ArdRQ}


def _ratio(group, err, tol):
    r = float(np.max(np.asarray(err) / np.asarray(tol)))
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"\n[{group}] worst err/tol {WORST[group]:.3g}")
    return r


def grad_tol(cond, ref):
    return max(1e-13, 64.0 * float(cond) * EPS * max(1.0, float(np.max(np.abs(ref)))))


def gram_tol(kind, logl, loga, x1, x2, Kd):
    """The bound of the Matern test with its exponent s replaced by alpha log1p(w): both sides round w in D steps
    (|dw| <= (D + 2) eps w, so |d log1p(w)| <= (D + 2) eps w / (1 + w) <= (D + 2) eps log1p(w) (1 + ...)), then log1p, the
    product with alpha and exp: |dK| / K <= about (D / 2 + 3) eps alpha log1p(w) + 8 eps per side."""
    D = x1.shape[1]
    s = np.exp(loga) * np.log1p(dk.scaled_sqdist(kind, dk.pack(kind, logl, loga=loga), x1, x2) / (2.0 * np.exp(loga)))
    return np.abs(Kd) * ((D + 6) * EPS * s + 16 * EPS) + 1e-300


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _data(seed, n, D, nt=100, dup=0):
    X = uniform(seed, 0, n * D).reshape((n, D), order="F")
    if dup:                    # the last `dup` rows repeat the first ones: w = 0 off the diagonal
        X[n - dup:] = X[:dup]
    y = np.sin(3 * X[:, 0]) + 0.3 * X[:, -1] + 0.1 * normal(seed + 1, 0, n)
    Xt = uniform(seed + 2, 0, nt * D).reshape((nt, D), order="F")
    return X, y, Xt


def _logl(kind, D):
    if not is_ard(kind):
        return np.log([0.35 * np.sqrt(D)])
    return np.log(0.35 * np.sqrt(D) * np.linspace(0.7, 1.4, D)) if D > 1 else np.log([0.35])


def _single(ctx, X, y, mean, kind, loghyp, logNoise):
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [mean])
    ctx.set_hyper(0, kind, np.concatenate([loghyp, [logNoise]]))
    return ctx.fit()


def _cond(g):
    ev = np.linalg.eigvalsh(g.F @ g.F.T)
    return ev[-1] / ev[0]


def _ng(kind, D):
    return (D if is_ard(kind) else 1) + 3


def _dense(X, y, mean, kind, h, ln):
    return DenseGP(kind, np.append(h, ln), X, y, mean)


@pytest.mark.parametrize("kind,D", list(itertools.product(KINDS, [1, 3, 8, 32, 33, 48])))
def test_kernel_matrix_against_the_dense_formula(ctx, kind, D):
    n1, n2 = 300, 131
    x1 = uniform(500 + D, 0, n1 * D).reshape((n1, D), order="F")
    x2 = uniform(600 + D, 0, n2 * D).reshape((n2, D), order="F")
    for la in np.log([0.3, 2.0, 50.0]):
        ll, ls = _logl(kind, D), 0.2
        ctx.set_train(x1, np.zeros(n1))
        ctx.set_hyper(0, kind, list(ll) + [la, ls, 0.0])
        K = ctx.kernel_matrix(0, x1, x2)
        Kd = dk.value(kind, dk.pack(kind, ll, ls, la), x1, x2)
        tol = gram_tol(kind, ll, la, x1, x2, Kd)
        _ratio("gram", np.abs(K - Kd), tol)
        assert np.all(np.abs(K - Kd) <= tol)
        Ks = ctx.kernel_matrix(0, x1, x1)
        assert np.array_equal(Ks, Ks.T)                            # bit-symmetric
        assert np.all(np.diag(Ks) == np.exp(2 * ls))               # k(x, x) = sigma^2 exactly


def test_large_alpha_bound_on_device_values(ctx):
    """With r^2 = sum u^2 / l^2: 0 <= k_RQ - k_SE <= k_SE (exp(r^4 / (8 alpha)) - 1) (log1p(w) >= w - w^2 / 2 with
    alpha w = r^2 / 2), against the product-form SE on the same device, at alpha = 1e6.  Rounding of either value: the bound
    of gram_tol."""
    D, n = 3, 200
    x = uniform(41, 0, n * D).reshape((n, D), order="F")
    ll, la, ls = np.log([0.4, 0.6, 0.9]), np.log(1e6), 0.1
    ctx.set_train(x, np.zeros(n))
    ctx.set_hyper(0, ARD_RQ, list(ll) + [la, ls, 0.0])
    ctx.set_hyper(1, 4, list(ll) + [ls, 0.0])
    Kr, Ks = ctx.kernel_matrix(0, x, x), ctx.kernel_matrix(1, x, x)
    r2 = dk.scaled_sqdist(ARD_RQ, dk.pack(ARD_RQ, ll, loga=la), x, x)
    slack = Ks * ((D + 6) * EPS * r2 + 32 * EPS)
    assert np.all(Kr - Ks >= -slack)
    assert np.all(Kr - Ks <= Ks * np.expm1(r2 * r2 / 8e6) + slack)


GOLDEN = load_cases()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_cases_through_every_call(ctx, name):
    """Every case of tests/golden/gp_rq.npz (50 digits) through kernel_matrix / fit / predict / gradients / loo / loo_gradients /
    predict_gradients, at the tolerances the rest of this file uses against the dense restatement."""
    c = GOLDEN[name]
    kind, cond, X, y, Xt = c["kind"], c["cond"], c["X"], c["y"], c["Xt"]
    n, D = X.shape
    nt = Xt.shape[0]
    h = np.concatenate([c["logl"], [c["loga"], c["logs"]]])
    ln = c["logNoise"]
    kss, noise = np.exp(2 * c["logs"]), np.exp(2 * ln)
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
    ctx.set_hyper(0, kind, np.append(h, ln))
    m = c["Kc"].shape[0]
    for K, Kg, x2 in ((ctx.kernel_matrix(0, X[:m], X[:m]), c["Kc"], X[:m]), (ctx.kernel_matrix(0, X[:m], Xt), c["Kt"], Xt)):
        tol = gram_tol(kind, c["logl"], c["loga"], X[:m], x2, Kg)
        _ratio("golden gram", np.abs(K - Kg), tol)
        assert np.all(np.abs(K - Kg) <= tol)
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    _ratio("golden mll", abs(mll[0] - c["mll"]), mll_tol(c["mll"], cond))
    assert abs(mll[0] - c["mll"]) <= mll_tol(c["mll"], cond)
    ctx.predict_run()
    mu, var = ctx.predict_fetch()
    tmu, tvar = moment_tol(c["mu"], c["var"], kss, noise, max(1.0, np.max(np.abs(y))))
    _ratio("golden moments", np.concatenate([np.abs(mu - c["mu"]) / tmu, np.abs(var - c["var"]) / tvar]), 1.0)
    assert np.all(np.abs(mu - c["mu"]) <= tmu) and np.all(np.abs(var - c["var"]) <= tvar)
    ng = _ng(kind, D)
    g = ctx.gradients(ng)[0]
    _ratio("golden grad", np.abs(g - c["grad"]), grad_tol(cond, c["grad"]))
    assert np.all(np.abs(g - c["grad"]) <= grad_tol(cond, c["grad"])), (g, c["grad"])
    lmu, lvar, lpd = ctx.loo()
    tm, tv, _, tsum = loo_tol(y, c["loo_mu"], c["loo_var"], np.full(n, kss), noise)
    _ratio("golden loo", np.concatenate([np.abs(lmu - c["loo_mu"]) / tm, np.abs(lvar - c["loo_var"]) / tv]), 1.0)
    assert np.all(np.abs(lmu - c["loo_mu"]) <= tm) and np.all(np.abs(lvar - c["loo_var"]) <= tv)
    assert abs(lpd[0] - c["lpd_sum"]) <= tsum
    lg, lp = ctx.loo_gradients(ng)
    _ratio("golden loo grad", np.abs(lg[0] - c["loo_grad"]), grad_tol(cond, c["loo_grad"]))
    assert np.all(np.abs(lg[0] - c["loo_grad"]) <= grad_tol(cond, c["loo_grad"])), (lg[0], c["loo_grad"])
    assert lp[0] == lpd[0]
    dmu, dvar = ctx.predict_gradients()
    he = np.append(np.broadcast_to(c["logl"], (D,)), c["logs"])      # the scales of the ArdSEProduct rule, as above
    tdm, tdv = pgd.tolerances(4, he, ln, X, y, Xt, c["dmu"], c["dvar"])
    _ratio("golden input gradients", np.concatenate([np.abs(dmu - c["dmu"]) / tdm, np.abs(dvar - c["dvar"]) / tdv]), 1.0)
    assert np.all(np.abs(dmu - c["dmu"]) <= tdm) and np.all(np.abs(dvar - c["dvar"]) <= tdv)


@pytest.mark.parametrize("kind,n,D", [(9, 515, 3), (10, 1400, 8), (10, 700, 5)])
def test_large_leaves_against_the_dense_restatement(ctx, kind, n, D):
    """Fused and classic steps and tile edges; test rows riding through the fit and the standalone sweep; mll and LOO gradients,
    LOO moments, the predictive covariance (symmetric to the bit) and the input gradients."""
    X, y, Xt = _data(700 + n + kind, n, D, nt=70, dup=7)
    Xt[5] = X[11]                                              # a test point on a training point
    ll, la, ls, ln, mean = _logl(kind, D), np.log(2.0), 0.1, np.log(0.25), float(np.mean(y))
    h = np.concatenate([ll, [la, ls]])
    r = _dense(X, y, mean, kind, h, ln)
    cond = _cond(r)
    nt = Xt.shape[0]
    mo, vo = r.prediction(Xt)
    go, lgo = r.grad(), r.loo_grad()
    lmu, lvar, lpd = r.loo()
    kss, noise = np.exp(2 * ls), np.exp(2 * ln)
    tmu, tvar = moment_tol(mo, vo, kss, noise, max(1.0, np.max(np.abs(y))))
    ng = _ng(kind, D)
    try:
        for fg, fs, ride in [(1, 1, 0), (1, 1, 1), (0, 0, 0), (1, 0, 1)]:
            ctx.set_option(hipabi.OPT_FUSED_GRAM, fg)
            ctx.set_option(hipabi.OPT_FUSED_STEPS, fs)
            ctx.set_train(X, y)
            ctx.set_leaves([0, n], np.arange(n), [0], [mean])
            ctx.set_hyper(0, kind, np.append(h, ln))
            if ride:
                ctx.set_test(Xt, [0, nt], np.arange(nt))
            mll, info, _ = ctx.fit()
            assert info[0] == 0
            _ratio("large leaves", abs(mll[0] - r.mll()), mll_tol(r.mll(), cond))
            assert abs(mll[0] - r.mll()) <= mll_tol(r.mll(), cond)
            if ride:
                ctx.predict_run()
                mu, var = ctx.predict_fetch()
            else:
                mu, var = ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
            _ratio("large leaves", np.concatenate([np.abs(mu - mo) / tmu, np.abs(var - vo) / tvar]), 1.0)
            assert np.all(np.abs(mu - mo) <= tmu) and np.all(np.abs(var - vo) <= tvar)
            g = ctx.gradients(ng)[0]
            _ratio("large leaves grad", np.abs(g - go), grad_tol(cond, go))
            assert np.all(np.abs(g - go) <= grad_tol(cond, go)), (g, go)
            lg, lp = ctx.loo_gradients(ng)
            _ratio("large leaves loo grad", np.abs(lg[0] - lgo), grad_tol(cond, lgo))
            assert np.all(np.abs(lg[0] - lgo) <= grad_tol(cond, lgo)), (lg[0], lgo)
            dmu_l, dvar_l, dlpd = ctx.loo()
            tm, tv, _, tsum = loo_tol(y, lmu, lvar, kss, noise)
            assert np.all(np.abs(dmu_l - lmu) <= tm) and np.all(np.abs(dvar_l - lvar) <= tv)
            assert abs(dlpd[0] - lpd) <= tsum and lp[0] == dlpd[0]
            S = ctx.predict_cov(0, nt)
            So = r.prediction_cov(Xt)
            assert np.array_equal(S, S.T)
            assert np.all(np.abs(S - So) <= np.max(tvar)), float(np.max(np.abs(S - So)))
            dmu, dvar = ctx.predict_gradients()
            dmo, dvo = r.input_gradients(Xt)
            # the scales of the ArdSEProduct rule at the same length-scales and sigma: |dk/dx_d| <= k |D_d| / l_d^2 there and here
            he = np.append(np.broadcast_to(ll, (D,)), ls)
            tdm, tdv = pgd.tolerances(4, he, ln, X, y, Xt, dmo, dvo)
            _ratio("input gradients", np.concatenate([np.abs(dmu - dmo) / tdm, np.abs(dvar - dvo) / tdv]), 1.0)
            assert np.all(np.abs(dmu - dmo) <= tdm) and np.all(np.abs(dvar - dvo) <= tdv)
            assert np.all(np.isfinite(dmu[5])) and np.all(np.isfinite(dvar[5]))
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)


def test_input_gradients_against_central_differences_of_device_predictions(ctx):
    n, D, nt = 300, 3, 12
    X, y, Xt = _data(2100, n, D, nt=nt)
    Xt[0] = X[3]
    h, ln, mean = np.concatenate([_logl(ARD_RQ, D), [np.log(0.3), 0.1]]), np.log(0.25), float(np.mean(y))
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [mean])
    ctx.set_hyper(0, ARD_RQ, np.append(h, ln))
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    ctx.fit()
    ctx.predict_run()
    dmu, dvar = ctx.predict_gradients()
    step = 1e-5
    for d in range(D):
        Xp, Xm = Xt.copy(), Xt.copy()
        Xp[:, d] += step
        Xm[:, d] -= step
        mp, vp = ctx.predict_leaves(Xp, [0, nt], np.arange(nt))
        mm, vm = ctx.predict_leaves(Xm, [0, nt], np.arange(nt))
        # truncation O(step^2 |f'''|) ~ 1e-10 x curvature scale 1 / l^3 ~ 1e2; rounding of two moments within 1e-11 over 2 step
        tol = 1e-6 * np.maximum(1.0, np.abs(dmu[:, d])) + 1e-11 / step
        assert np.all(np.abs((mp - mm) / (2 * step) - dmu[:, d]) <= tol)
        tol = 1e-6 * np.maximum(1.0, np.abs(dvar[:, d])) + 1e-11 / step
        assert np.all(np.abs((vp - vm) / (2 * step) - dvar[:, d]) <= tol)


@pytest.mark.parametrize("n,D", [(515, 3), (1300, 8), (400, 36), (100, 1)])
def test_ard_with_equal_lengthscales_is_the_iso_kind_bit_for_bit(ctx, n, D):
    """The iso kind fills its factor table with D copies of 1 / (2 alpha l^2): the ARD kind with every l_d = l runs the same
    operations, so mll, the factor, moments, da, ds and dnoise are equal to the bit, and the iso dl is the ARD dl_d summed in
    ascending d."""
    X, y, Xt = _data(900 + n, n, D)
    ln, mean, l0, la, ls = np.log(0.3), float(np.mean(y)), np.log(0.4 * np.sqrt(D)), np.log(1.5), 0.3
    mi = _single(ctx, X, y, mean, ISO_RQ, np.array([l0, la, ls]), ln)[0][0]
    Fi = ctx.download_factor(0, n)[0]
    mui, vari = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    gi = ctx.gradients(4)[0]
    lgi = ctx.loo_gradients(4)[0][0]
    ma = _single(ctx, X, y, mean, ARD_RQ, np.concatenate([np.full(D, l0), [la, ls]]), ln)[0][0]
    Fa = ctx.download_factor(0, n)[0]
    mua, vara = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    ga = ctx.gradients(D + 3)[0]
    lga = ctx.loo_gradients(D + 3)[0][0]
    assert ma == mi and np.array_equal(Fa, Fi)
    assert np.array_equal(mua, mui) and np.array_equal(vara, vari)
    for a, i in ((ga, gi), (lga, lgi)):
        sl = 0.0
        for v in a[:D]:
            sl += v
        assert np.array_equal(np.array([sl, a[D], a[D + 1], a[D + 2]]), i), (sl, a[D:], i)


@pytest.mark.parametrize("kind,D", list(itertools.product(KINDS, [1, 8, 35, 36, 48])))
def test_gradients_against_the_dense_trace_and_finite_differences(ctx, kind, D):
    n = 300
    X, y, _ = _data(1100 + D + 10 * kind, n, D, nt=4, dup=12)
    ll, la, ls, ln, mean = _logl(kind, D), np.log(0.8), 0.1, np.log(0.25), float(np.mean(y))
    h = np.concatenate([ll, [la, ls]])
    _single(ctx, X, y, mean, kind, h, ln)
    ng = _ng(kind, D)
    g = ctx.gradients(ng)[0]
    lg = ctx.loo_gradients(ng)[0][0]
    dg = _dense(X, y, mean, kind, h, ln)
    go, lgo = dg.grad(), dg.loo_grad()
    assert np.all(np.isfinite(g)) and np.all(np.isfinite(lg))
    tg = grad_tol(_cond(dg), go)
    _ratio("gradients dense", np.abs(g - go), tg)
    assert np.all(np.abs(g - go) <= tg), (g, go)
    tl = grad_tol(_cond(dg), lgo)
    _ratio("loo gradients dense", np.abs(lg - lgo), tl)
    assert np.all(np.abs(lg - lgo) <= tl), (lg, lgo)
    full = np.append(h, ln)
    nl = ng - 3

    def values(hh):
        m = _single(ctx, X, y, mean, kind, hh[:-1], hh[-1])[0][0]
        return np.array([m, ctx.loo()[2][0]])

    def central(j, step):
        hp, hm = full.copy(), full.copy()
        hp[j] += step
        hm[j] -= step
        return (values(hp) - values(hm)) / (2 * step)

    step = 1e-4
    scale = max(1.0, abs(dg.mll()), abs(dg.loo()[2]))
    for j in sorted(set([0, nl // 2, nl - 1, nl, nl + 1, nl + 2])):
        fd, fd2 = central(j, step), central(j, step / 2)
        for which, dev in ((0, g), (1, lg)):
            # truncation of fd2: (fd - fd2) / 3 (Richardson), bounded by |fd - fd2|; rounding of the two values, each within
            # 64 n eps max(1, |value|) (backward-stable Cholesky and log-determinant), divided by the step
            tol = 1e-7 * max(1.0, abs(fd2[which])) + abs(fd[which] - fd2[which]) + 64 * n * EPS * scale / step
            assert tol <= 1e-4 * max(1.0, abs(fd2[which])), (j, tol, fd2)      # tight enough to catch a wrong factor
            _ratio("finite differences", abs(dev[j] - fd2[which]), tol)
            assert abs(dev[j] - fd2[which]) <= tol, (which, j, dev[j], fd2[which])


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_on_copy_and_prefix_leaves_and_under_a_leaf_mask(ctx, kind):
    """Leaf 0 (300 rows), leaf 1 = COPY of it (same mean: shares its sums), leaf 2 = COPY with a mean of its own, leaf 3 =
    PREFIX: 600 rows whose first 300 are leaf 0's (factor continued from column 300)."""
    n, D = 600, 5
    X, y, _ = _data(1400 + kind, n, D, nt=4)
    h, ln = np.concatenate([_logl(kind, D), [np.log(3.0), 0.0]]), np.log(0.3)
    means = [0.1, 0.1, -0.4, 0.2]
    rows = [np.arange(300), np.arange(300), np.arange(300), np.arange(n)]
    ptr = np.cumsum([0] + [r.size for r in rows])
    ng = _ng(kind, D)
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.concatenate(rows), [0, 0, 0, 0], means)
    ctx.set_hyper(0, kind, np.append(h, ln))
    ctx.set_sharing([0, 1, 1, 2], [-1, 0, 0, 0], [0, 0, 0, 300])
    mll, info, _ = ctx.fit()
    assert np.all(info == 0)
    g = ctx.gradients(ng)
    lg = ctx.loo_gradients(ng)[0]
    for l in range(4):
        r = _dense(X[rows[l]], y[rows[l]], means[l], kind, h, ln)
        cond = _cond(r)
        assert abs(mll[l] - r.mll()) <= mll_tol(r.mll(), cond)
        go, lgo = r.grad(), r.loo_grad()
        _ratio("copy/prefix/mask", np.abs(g[l] - go), grad_tol(cond, go))
        assert np.all(np.abs(g[l] - go) <= grad_tol(cond, go)), (l, g[l], go)
        assert np.all(np.abs(lg[l] - lgo) <= grad_tol(cond, lgo)), (l, lg[l], lgo)
    nl = ng - 2
    assert np.array_equal(g[0][:nl], g[1][:nl])                # copygradients: the source's contraction sums, da included
    for mask in ([0, 1, 0, 1], [0, 0, 1, 0], [1, 0, 0, 0]):
        ctx.set_gradient_leaves(mask)
        gm = ctx.gradients(ng)
        for l in range(4):
            if mask[l]:     # another task list: the per-task sums are added in another order
                assert np.allclose(gm[l], g[l], rtol=1e-12, atol=1e-14 * np.max(np.abs(g[l]))), (mask, l)
            else:
                assert np.all(gm[l] == 0.0)
    ctx.set_gradient_leaves(None)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_leave_a_usable_context(ctx, kind):
    n, D = 200, 3
    X, y, _ = _data(1500, n, D, nt=4)
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
    ln = np.log(0.3)
    nlen = D if is_ard(kind) else 1
    good = [0.1, 0.2, 0.3][:nlen] + [0.5, 0.0, ln]
    bads = [good[1:], [0.1] + good, good[:nlen] + [np.nan, 0.0, ln]]   # one value short, one too many, loga = nan
    for bad in bads:
        with pytest.raises(hipabi.DsmgpError) as e:
            ctx.set_hyper(0, kind, bad)
        assert e.value.code == -1                               # DSMGP_E_ARG
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.set_hyper(0, 11, good)                              # no kind 11
    assert e.value.code == -1
    ctx.set_hyper(0, kind, good)
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    r = _dense(X, y, 0.0, kind, np.array(good[:-1]), ln)
    assert abs(mll[0] - r.mll()) <= mll_tol(r.mll(), _cond(r))


def test_one_context_with_every_kind_equals_each_leaf_alone(ctx):
    """All eleven kinds side by side in one context (kernel id = kind), each leaf against the same leaf in a context of its own."""
    D = 4
    X, y, _ = _data(1600, 2200, D, nt=4)
    bounds = np.linspace(0, 2200, 12).astype(int)
    rows = [np.arange(bounds[i], bounds[i + 1]) for i in range(11)]
    la = np.log(np.array([0.5, 0.7, 0.9, 1.2]))
    hyp = [(0, np.array([np.log(0.5), 0.1])), (1, np.append(la, 0.0)), (2, np.array([np.log(1.5), 0.0])),
           (3, np.append(la, 0.0)), (4, np.append(la, -0.1)), (5, np.array([np.log(0.6), 0.1])),
           (6, np.array([np.log(0.6), -0.1])), (7, np.append(la, 0.2)), (8, np.append(la, 0.0)),
           (9, np.array([np.log(0.6), np.log(0.7), 0.1])), (10, np.concatenate([la, [np.log(4.0), -0.1]]))]
    ln = np.log(0.3)
    means = [0.05 * i - 0.2 for i in range(11)]
    ptr = np.cumsum([0] + [r.size for r in rows])
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.concatenate(rows), list(range(11)), means)
    for k, (kind, h) in enumerate(hyp):
        ctx.set_hyper(k, kind, np.append(h, ln))
    mll, info, _ = ctx.fit()
    assert np.all(info == 0)
    g = ctx.gradients(D + 3)
    lg = ctx.loo_gradients(D + 3)[0]
    c2 = hipabi.Context(0)
    try:
        for l, (kind, h) in enumerate(hyp):
            ml = _single(c2, X[rows[l]], y[rows[l]], means[l], kind, h, ln)[0][0]
            gl = c2.gradients(D + 3)[0]
            lgl = c2.loo_gradients(D + 3)[0][0]
            assert abs(mll[l] - ml) <= 1e-12 * max(1.0, abs(ml)), l
            assert np.allclose(g[l], gl, rtol=1e-12, atol=1e-13 * max(1.0, np.max(np.abs(gl)))), l
            assert np.allclose(lg[l], lgl, rtol=1e-12, atol=1e-13 * max(1.0, np.max(np.abs(lgl)))), l
            assert np.all(g[l][h.size + 1:] == 0.0) and np.all(lg[l][h.size + 1:] == 0.0)     # zeros past the hyper-vector
            if kind >= 9:
                r = _dense(X[rows[l]], y[rows[l]], means[l], kind, h, ln)
                go = r.grad()
                _ratio("eleven kinds", np.abs(g[l][:go.size] - go), grad_tol(_cond(r), go))
                assert np.all(np.abs(g[l][:go.size] - go) <= grad_tol(_cond(r), go)), (l, g[l], go)
    finally:
        c2.close()


def _dense_leaves(m, X, y):
    return [DenseGP(lf.kernel.kind, dk.pack(lf.kernel.kind, lf.kernel.logl, lf.kernel.logs, lf.kernel.loga, lf.logNoise), X[lf.obs], y[lf.obs], lf.mean.m)
            for lf in ptree.get_leaves(m.root)]


def _rbcm(root, gps, x, s):
    C = 1.0 / s
    mu = np.zeros(x.shape[0])
    for c in root.children:
        m_, t_ = ospn._predict_poe(c, gps, x)
        beta = 0.5 * (np.log(s) - np.log(1.0 / t_))
        C = C + beta * t_ - beta / s
        mu = mu + m_ * (beta * t_)
    return mu / C, 1.0 / C


@pytest.mark.parametrize("family,kind", [("dsmgp", 10), ("dsmgp", 9), ("dsmgp_depth4", 10), ("poe", 9), ("rbcm", 10)])
def test_whole_models_against_dense_leaves(family, kind):
    N, D = 3000, 4
    X, y, Xt = regression_data(N, D, n_test=200, seed=910)
    ll, la, ls, ln = (np.log([0.5, 0.7, 0.9, 1.2]) if is_ard(kind) else np.log(0.8)), np.log(1.5), 0.1, np.log(0.2)
    k = CLASSES[kind](ll, la, ls)
    mf = dsm.ConstMean(float(np.mean(y)))
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 3, 4, M=60, kernel=k, logNoise=ln, seed=4)
    elif family == "dsmgp_depth4":
        m = dsm.buildDSMGP(X, y, 2, 4, M=8, D=4, kernel=k, logNoise=ln, seed=9)
    elif family == "poe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=k, meanFun=mf, logNoise=ln, seed=4)
    else:
        m = dsm.buildBCM(X, y, 8, M=100, kernel=k, logNoise=ln, seed=4)
    gps = _dense_leaves(m, X, y)
    conds = np.array([_cond(g) for g in gps])
    ref = np.array([g.mll() for g in gps])
    assert np.all(np.abs(m.leaf_mll - ref) <= mll_tol(ref, conds))
    mu, var = dsm.predict(m, Xt)
    if family.startswith("dsmgp"):
        mo, vo = ospn.predict(m.root, gps, Xt)
    elif family == "poe":
        mo, vo = ospn.predict_poe(m.root, gps, Xt)
    else:          # the rBCM prior variance is k(x*, x*) + noise = sigma^2 + noise
        mo, vo = _rbcm(m.root, gps, Xt, np.full(Xt.shape[0], np.exp(2 * ls) + np.exp(2 * ln)))
    tmu, tvar = moment_tol(mo, vo, np.exp(2 * ls), np.exp(2 * ln), max(1.0, np.max(np.abs(y))))
    _ratio("whole models", np.concatenate([np.abs(mu - mo) / tmu, np.abs(var - vo) / tvar]), 1.0)
    assert np.all(np.abs(mu - mo) <= tmu) and np.all(np.abs(var - vo) <= tvar)
    g = dsm.updategradients(m).copy()
    ng = _ng(kind, D)
    for l, r in enumerate(gps):
        go = r.grad()
        assert np.all(np.abs(g[l, :ng] - go) <= grad_tol(conds[l], go)), l
    k0 = m.leaves[0].kernel
    assert isinstance(k0.da, float) and isinstance(k0.ds, float) and k0.da == g[0, ng - 3] and k0.ds == g[0, ng - 2]
    assert k0.dl.shape == (D,) if is_ard(kind) else isinstance(k0.dl, float)


def test_mixed_kernel_vector_and_n_sub():
    N, D = 2000, 3
    X, y, Xt = regression_data(N, D, n_test=150, seed=930)
    kern = [dsm.IsoSE(np.log(0.4), 0.0), dsm.ArdRQ(np.log([0.4, 0.6, 0.9]), np.log(2.0), 0.1)]
    kw = dict(M=60, logNoise=np.log(0.2), seed=5)
    m = dsm.buildDSMGP(X, y, 2, 4, kernel=kern, **kw)
    kinds = [lf.kernel.kind for lf in m.leaves]
    assert 0 in kinds and 10 in kinds
    mu, var = dsm.predict(m, Xt)
    mr = dsm.buildDSMGP(X, y, 2, 4, kernel=kern, fit_now=False, **kw)
    dsm.resident_test(mr, Xt)
    dsm.fit(mr)
    mur, varr = dsm.predict(mr, Xt)
    assert np.allclose(mur, mu, rtol=1e-11, atol=1e-13) and np.allclose(varr, var, rtol=1e-11, atol=1e-13)
    p = dsm.getparams(m)
    dsm.setparams(m, p)
    assert np.array_equal(dsm.getparams(m), p)
    m2 = dsm.buildDSMGP(X, y, 2, 4, kernel=kern, n_sub=2, **kw)
    assert np.allclose(m2.leaf_mll, m.leaf_mll, rtol=1e-12, atol=0)
    dsm.updategradients(m)
    dsm.updategradients(m2)
    assert np.allclose(dsm.grad_mll(m), dsm.grad_mll(m2), rtol=1e-10, atol=1e-12)


def test_train_follows_a_dense_loop_and_moves_the_shape():
    N, D = 1500, 3
    X = uniform(77, 0, N * D).reshape((N, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.05 * normal(78, 0, N)
    kw = dict(M=200, logNoise=np.log(0.1), seed=3)
    m = dsm.buildDSMGP(X, y, 2, 2, kernel=dsm.ArdRQ(np.log([0.3, 0.5, 0.5]), np.log(1.0), 0.0), **kw)
    h = dsm.getparams(m).copy()
    opt = dsm.ADAM(eta=0.05)
    ref = h.copy()
    for _ in range(3):
        dsm.setparams(m, ref)
        dsm.fit(m)
        gps = _dense_leaves(m, X, y)
        for l, r in enumerate(gps):
            assert abs(m.leaf_mll[l] - r.mll()) <= mll_tol(r.mll(), _cond(r))
        m.leaf_grad = np.array([r.grad() for r in gps])
        ref = ref + opt.apply(ref, dsm.grad_mll(m))
    dsm.setparams(m, h)
    dsm.fit(m)
    dsm.train(m, dsm.ADAM(eta=0.05), iterations=3, randinit=False)
    out = dsm.getparams(m)
    assert np.allclose(out, ref, rtol=1e-9, atol=1e-12), (out, ref)
    assert out.size == D + 3 and out[D] != h[D]                # loga moved
    mi = dsm.buildDSMGP(X, y, 2, 2, kernel=dsm.IsoRQ(np.log(0.3), np.log(1.0), 0.0), **kw)
    hi = dsm.getparams(mi).copy()
    opt = dsm.ADAM(eta=0.05)
    ref = hi.copy()
    for _ in range(3):             # the LOO loop: dense densities and their gradients (eq. 5.13) through grad_loo
        dsm.setparams(mi, ref)
        dsm.fit(mi)
        gps = _dense_leaves(mi, X, y)
        mi.leaf_lpd = np.array([r.loo()[2] for r in gps])
        mi.leaf_grad = np.array([r.loo_grad() for r in gps])
        ref = ref + opt.apply(ref, dsm.grad_loo(mi))
    dsm.setparams(mi, hi)
    dsm.fit(mi)
    dsm.train(mi, dsm.ADAM(eta=0.05), iterations=3, randinit=False, objective="loo")
    out = dsm.getparams(mi)
    assert np.allclose(out, ref, rtol=1e-9, atol=1e-12), (out, ref)
    assert out.size == 4 and out[1] != hi[1]                   # loga moved


def test_a_pooled_context_takes_an_rq_kind_after_set_test():
    """Under a device pool set_test builds the fused step lists at once, before any kernel id is set.  The rational quadratic
    kind set afterwards -- and a later swap of which id has it -- must still reach the diagonal blocks of its leaves
    (diag_fused_reg_rq_kernel is launched only while such an id exists).  40 leaves of 200 rows: both block steps run fused."""
    L, nl, D = 40, 200, 3
    X, y, Xt = _data(1700, L * nl, D, nt=60)
    nt = Xt.shape[0]
    rows = [np.arange(l * nl, (l + 1) * nl) for l in range(L)]
    ptr = np.cumsum([0] + [nl] * L)
    kid = [l % 2 for l in range(L)]
    means = [float(np.mean(y[r])) for r in rows]
    rptr, ridx = np.arange(L + 1) * nt, np.tile(np.arange(nt), L)
    ln = np.log(0.3)
    rq = np.concatenate([np.log([0.5, 0.7, 0.9]), [np.log(1.2), 0.1]])
    se = np.array([np.log(0.4), 0.0])
    c = hipabi.Context(0)
    try:
        c.reserve(1 << 30)
        c.set_train(X, y)
        c.set_leaves(ptr, np.concatenate(rows), kid, means)
        c.set_test(Xt, rptr, ridx)                             # pooled: the joint step lists are built here
        for hyp in ({0: (10, rq), 1: (0, se)}, {0: (0, se), 1: (9, np.array([np.log(0.6), np.log(0.5), 0.2]))}):
            for k, (kind, h) in hyp.items():
                c.set_hyper(k, kind, np.append(h, ln))
            mll, info, _ = c.fit()
            assert np.all(info == 0)
            c.predict_run()
            mu, var = c.predict_fetch()
            for l in (0, 1, L - 2, L - 1):
                kind, h = hyp[kid[l]]
                if kind >= 9:
                    r = _dense(X[rows[l]], y[rows[l]], means[l], kind, h, ln)
                    _ratio("pooled set_test", abs(mll[l] - r.mll()), mll_tol(r.mll(), _cond(r)))
                    assert abs(mll[l] - r.mll()) <= mll_tol(r.mll(), _cond(r)), l
                    mo, vo = r.prediction(Xt)
                    tmu, tvar = moment_tol(mo, vo, np.exp(2 * h[-1]), np.exp(2 * ln), max(1.0, np.max(np.abs(y))))
                    assert np.all(np.abs(mu[rptr[l]:rptr[l + 1]] - mo) <= tmu) and np.all(np.abs(var[rptr[l]:rptr[l + 1]] - vo) <= tvar)
    finally:
        c.close()
