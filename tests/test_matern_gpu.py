"""GPU suite for the Matern kernels (DSMGP kinds 5-8): Gram tiles, single leaves and gradients against the 50-digit references of
tests/golden/gp_matern.npz and the dense restatement of tests/dense_gp.py, the iso kind as the ARD kind with equal
length-scales (bit for bit), gradients by central differences at D up to 48 with duplicate training points, COPY / PREFIX
leaves and masks, all nine kinds in one context, whole models, mixed kernel vectors with resident test rows and n_sub = 2,
train! and the refusals.  Tolerances come from tests/pred_tolerance.py (mll_tol, moment_tol) and the gradient rule
64 cond_2(K_y) eps max(1, |g|_inf) of tests/test_gradients_gpu.py; every group prints its worst err/tol."""
import itertools
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi, tree as ptree
from deepstructuredmixtures_amd.datagen import uniform, normal, regression_data
from oracle import spn as ospn
import dense_kernels as dk
from dense_gp import DenseGP
from pred_tolerance import EPS, mll_tol, moment_tol

pytestmark = pytest.mark.gpu

KINDS = dk.MATERN


def is_ard(kind):
    return kind in dk.ARD


GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_matern.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files})
WORST = {}
CLASSES = {5: dsm.IsoMatern32, 6: dsm.IsoMatern52, 7: dsm.ArdMatern32, 8: dsm.ArdMatern52}


def _case(name):
    return {k.split("/")[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}


def _ratio(group, err, tol):
    r = float(np.max(np.asarray(err) / np.asarray(tol)))
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"\n[{group}] worst err/tol {WORST[group]:.3g}")
    return r


def grad_tol(cond, ref):
    return max(1e-13, 64.0 * float(cond) * EPS * max(1.0, float(np.max(np.abs(ref)))))


def gram_tol(kind, logl, x1, x2, Kd):
    """Both sides round s^2 in D steps (|dz| <= (D + 2) eps z), then sqrt, exp(-s) and the polynomial: |dK| / K <= about
    (D / 2 + 3) eps s + 8 eps per side."""
    D = x1.shape[1]
    s = np.sqrt(dk.two_nu(kind) * dk.scaled_sqdist(kind, dk.pack(kind, logl), x1, x2))
    return np.abs(Kd) * ((D + 6) * EPS * s + 16 * EPS) + 1e-300


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _data(seed, n, D, nt=100, dup=0):
    X = uniform(seed, 0, n * D).reshape((n, D), order="F")
    if dup:                    # the last `dup` rows repeat the first ones: s = 0 off the diagonal
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
    return (D if is_ard(kind) else 1) + 2


@pytest.mark.parametrize("kind,D", list(itertools.product(KINDS, [1, 3, 8, 32, 33, 48])))
def test_kernel_matrix_against_the_dense_formula(ctx, kind, D):
    n1, n2 = 300, 131
    x1 = uniform(500 + D, 0, n1 * D).reshape((n1, D), order="F")
    x2 = uniform(600 + D, 0, n2 * D).reshape((n2, D), order="F")
    ll, ls = _logl(kind, D), 0.2
    ctx.set_train(x1, np.zeros(n1))
    ctx.set_hyper(0, kind, list(ll) + [ls, 0.0])
    K = ctx.kernel_matrix(0, x1, x2)
    Kd = dk.value(kind, dk.pack(kind, ll, ls), x1, x2)
    tol = gram_tol(kind, ll, x1, x2, Kd)
    _ratio("gram", np.abs(K - Kd), tol)
    assert np.all(np.abs(K - Kd) <= tol)
    Ks = ctx.kernel_matrix(0, x1, x1)
    assert np.array_equal(Ks, Ks.T)                            # bit-symmetric
    assert np.all(np.diag(Ks) == np.exp(2 * ls))               # k(x, x) = sigma^2


@pytest.mark.parametrize("name", CASES)
def test_single_leaf_against_50_digit_references(ctx, name):
    c = _case(name)
    kind = int(c["kind"])
    X, y, Xt = c["X"], c["y"], c["Xt"]
    h = np.append(c["logl"], float(c["logs"]))
    m = min(X.shape[0], 8)
    ctx.set_train(X, y)
    ctx.set_hyper(0, kind, np.append(h, float(c["logNoise"])))
    Kc = ctx.kernel_matrix(0, X[:m], X[:m])
    Kt = ctx.kernel_matrix(0, X[:m], Xt)
    tolK = gram_tol(kind, c["logl"], X[:m], X[:m], c["Kc"])
    _ratio("golden K", np.abs(Kc - c["Kc"]), tolK)
    assert np.all(np.abs(Kc - c["Kc"]) <= tolK)
    assert np.all(np.abs(Kt - c["Kt"]) <= gram_tol(kind, c["logl"], X[:m], Xt, c["Kt"]))
    nt = Xt.shape[0]
    kss = np.exp(2 * float(c["logs"]))
    noise = np.exp(2 * float(c["logNoise"]))
    tmu, tvar = moment_tol(c["mu"], c["var"], kss, noise, max(1.0, float(np.max(np.abs(y)))))
    tml = mll_tol(float(c["mll"]), float(c["cond"]))
    tg = grad_tol(c["cond"], c["grad"])
    try:
        for fg, fs, lanes in itertools.product([1, 0], [1, 0], [1, 2]):
            ctx.set_option(hipabi.OPT_FUSED_GRAM, fg)
            ctx.set_option(hipabi.OPT_FUSED_STEPS, fs)
            ctx.set_option(hipabi.OPT_LANES, lanes)
            mll, info, _ = _single(ctx, X, y, float(c["mean"]), kind, h, float(c["logNoise"]))
            assert info[0] == 0
            _ratio("golden mll", abs(mll[0] - c["mll"]), tml)
            assert abs(mll[0] - c["mll"]) <= tml, (fg, fs, lanes, mll[0], float(c["mll"]))
            mu, var = ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
            _ratio("golden moments", np.concatenate([np.abs(mu - c["mu"]) / tmu, np.abs(var - c["var"]) / tvar]), 1.0)
            assert np.all(np.abs(mu - c["mu"]) <= tmu) and np.all(np.abs(var - c["var"]) <= tvar), (fg, fs, lanes)
            g = ctx.gradients(c["grad"].size)[0]
            _ratio("golden gradients", np.abs(g - c["grad"]), tg)
            assert np.all(np.abs(g - c["grad"]) <= tg), (fg, fs, lanes, g, c["grad"])
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)


@pytest.mark.parametrize("kind,n,D", [(6, 515, 3), (7, 1400, 8), (8, 1400, 5), (5, 700, 4)])
def test_large_leaves_against_the_dense_restatement(ctx, kind, n, D):
    """Leaves beyond what the 50-digit references hold (several hundred rows and above 1300: the classic steps and the update
    kernel), against the dense restatement that tests/test_matern_host.py pins to those references."""
    X, y, Xt = _data(700 + n + kind, n, D, dup=7)
    ll, ls, ln, mean = _logl(kind, D), 0.1, np.log(0.25), float(np.mean(y))
    h = np.append(ll, ls)
    r = DenseGP(kind, dk.pack(kind, ll, ls, logNoise=ln), X, y, mean)
    cond = _cond(r)
    mo, vo = r.prediction(Xt)
    go = r.grad()
    tmu, tvar = moment_tol(mo, vo, np.exp(2 * ls), np.exp(2 * ln), max(1.0, np.max(np.abs(y))))
    try:
        for fg, fs in itertools.product([1, 0], [1, 0]):
            ctx.set_option(hipabi.OPT_FUSED_GRAM, fg)
            ctx.set_option(hipabi.OPT_FUSED_STEPS, fs)
            mll, info, _ = _single(ctx, X, y, mean, kind, h, ln)
            assert info[0] == 0
            _ratio("large leaves", abs(mll[0] - r.mll()), mll_tol(r.mll(), cond))
            assert abs(mll[0] - r.mll()) <= mll_tol(r.mll(), cond)
            mu, var = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
            _ratio("large leaves", np.concatenate([np.abs(mu - mo) / tmu, np.abs(var - vo) / tvar]), 1.0)
            assert np.all(np.abs(mu - mo) <= tmu) and np.all(np.abs(var - vo) <= tvar)
            g = ctx.gradients(_ng(kind, D))[0]
            _ratio("large leaves", np.abs(g - go), grad_tol(cond, go))
            assert np.all(np.abs(g - go) <= grad_tol(cond, go)), (g, go)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)


@pytest.mark.parametrize("iso,n,D", [(5, 515, 3), (6, 1300, 8), (6, 400, 36), (5, 100, 1)])
def test_ard_with_equal_lengthscales_is_the_iso_kind_bit_for_bit(ctx, iso, n, D):
    """The iso kind fills its factor table with D copies of 2 nu / l^2: the ARD kind with every l_d = l runs the same
    operations, so mll, moments, ds and dnoise are equal to the bit, and the iso dl is the ARD dl_d summed in ascending d."""
    X, y, Xt = _data(900 + n, n, D)
    ln, mean, l0, ls = np.log(0.3), float(np.mean(y)), np.log(0.4 * np.sqrt(D)), 0.3
    mi = _single(ctx, X, y, mean, iso, np.array([l0, ls]), ln)[0][0]
    mui, vari = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    gi = ctx.gradients(3)[0]
    ma = _single(ctx, X, y, mean, iso + 2, np.append(np.full(D, l0), ls), ln)[0][0]
    mua, vara = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    ga = ctx.gradients(D + 2)[0]
    assert ma == mi
    assert np.array_equal(mua, mui) and np.array_equal(vara, vari)
    sl = 0.0
    for v in ga[:D]:
        sl += v
    assert np.array_equal(np.array([sl, ga[D], ga[D + 1]]), gi), (sl, ga[D:], gi)
    Ki = ctx.kernel_matrix(0, X[:50], Xt[:30])
    ctx.set_hyper(0, iso, np.array([l0, ls, ln]))
    assert np.array_equal(ctx.kernel_matrix(0, X[:50], Xt[:30]), Ki)
    _ratio("iso identity", 0.0, 1.0)


@pytest.mark.parametrize("kind,D", list(itertools.product(KINDS, [1, 8, 35, 36, 48])))
def test_gradients_against_the_dense_trace_and_finite_differences(ctx, kind, D):
    n = 300
    X, y, _ = _data(1100 + D + 10 * kind, n, D, nt=4, dup=12)
    ll, ls, ln, mean = _logl(kind, D), 0.1, np.log(0.25), float(np.mean(y))
    h = np.append(ll, ls)
    _single(ctx, X, y, mean, kind, h, ln)
    ng = _ng(kind, D)
    g = ctx.gradients(ng)[0]
    dg = DenseGP(kind, dk.pack(kind, ll, ls, logNoise=ln), X, y, mean)
    go = dg.grad()
    assert np.all(np.isfinite(g))
    tg = grad_tol(_cond(dg), go)
    _ratio("gradients dense", np.abs(g - go), tg)
    assert np.all(np.abs(g - go) <= tg), (g, go)
    full = np.append(h, ln)
    nl = ng - 2

    def central(j, step):
        hp, hm = full.copy(), full.copy()
        hp[j] += step
        hm[j] -= step
        return (_single(ctx, X, y, mean, kind, hp[:-1], hp[-1])[0][0] - _single(ctx, X, y, mean, kind, hm[:-1], hm[-1])[0][0]) / (2 * step)

    step = 1e-4
    for j in sorted(set([0, nl // 2, nl - 1, nl, nl + 1])):
        fd, fd2 = central(j, step), central(j, step / 2)
        # truncation of fd2: (fd - fd2) / 3 (Richardson), bounded by |fd - fd2|; rounding of the two mll values, each within
        # 64 n eps max(1, |mll|) (backward-stable Cholesky and log-determinant), divided by the step
        tol = 1e-7 * max(1.0, abs(fd2)) + abs(fd - fd2) + 64 * n * EPS * max(1.0, abs(dg.mll())) / step
        assert tol <= 1e-4 * max(1.0, abs(fd2)), (j, tol, fd2)      # tight enough to catch a wrong per-dimension factor
        _ratio("finite differences", abs(g[j] - fd2), tol)
        assert abs(g[j] - fd2) <= tol, (j, g[j], fd2)


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_on_copy_and_prefix_leaves_and_under_a_leaf_mask(ctx, kind):
    """Leaf 0 (300 rows), leaf 1 = COPY of it (same mean: shares its sums), leaf 2 = COPY with a mean of its own, leaf 3 =
    PREFIX: 600 rows whose first 300 are leaf 0's (factor continued from column 300)."""
    n, D = 600, 5
    X, y, _ = _data(1400 + kind, n, D, nt=4)
    ll, ls, ln = _logl(kind, D), 0.0, np.log(0.3)
    means = [0.1, 0.1, -0.4, 0.2]
    rows = [np.arange(300), np.arange(300), np.arange(300), np.arange(n)]
    ptr = np.cumsum([0] + [r.size for r in rows])
    ng = _ng(kind, D)
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.concatenate(rows), [0, 0, 0, 0], means)
    ctx.set_hyper(0, kind, np.concatenate([ll, [ls, ln]]))
    ctx.set_sharing([0, 1, 1, 2], [-1, 0, 0, 0], [0, 0, 0, 300])
    mll, info, _ = ctx.fit()
    assert np.all(info == 0)
    g = ctx.gradients(ng)
    for l in range(4):
        r = DenseGP(kind, dk.pack(kind, ll, ls, logNoise=ln), X[rows[l]], y[rows[l]], means[l])
        cond = _cond(r)
        assert abs(mll[l] - r.mll()) <= mll_tol(r.mll(), cond)
        go = r.grad()
        _ratio("copy/prefix/mask", np.abs(g[l] - go), grad_tol(cond, go))
        assert np.all(np.abs(g[l] - go) <= grad_tol(cond, go)), (l, g[l], go)
    nl = ng - 2
    assert np.array_equal(g[0][:nl], g[1][:nl])                # copygradients: the source's contraction sums
    assert np.allclose(g[0], g[1], rtol=1e-12, atol=0), (g[0] - g[1])
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
    bads = ([0.1, 0.2, 0.0, np.log(0.3)], [0.1, 0.2, 0.3, 0.4, 0.0, np.log(0.3)]) if is_ard(kind) else \
        ([0.1, 0.2, 0.0, np.log(0.3)], [0.1, 0.2, 0.3, 0.0, np.log(0.3)])
    for bad in bads:
        with pytest.raises(hipabi.DsmgpError) as e:
            ctx.set_hyper(0, kind, bad)
        assert e.value.code == -1                               # DSMGP_E_ARG
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.set_hyper(0, 9, [0.1, 0.0, np.log(0.3)])              # no kind 9
    assert e.value.code == -1
    ll = [0.1, 0.2, 0.3] if is_ard(kind) else [0.2]
    ctx.set_hyper(0, kind, ll + [0.0, np.log(0.3)])
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    r = DenseGP(kind, dk.pack(kind, ll, 0.0, logNoise=np.log(0.3)), X, y, 0.0)
    assert abs(mll[0] - r.mll()) <= mll_tol(r.mll(), _cond(r))


def test_one_context_with_every_kind_equals_each_leaf_alone(ctx):
    """All nine kinds side by side in one context (kernel id = kind), each leaf against the same leaf in a context of its own."""
    D = 4
    X, y, _ = _data(1600, 1800, D, nt=4)
    bounds = np.linspace(0, 1800, 10).astype(int)
    rows = [np.arange(bounds[i], bounds[i + 1]) for i in range(9)]
    la = np.log(np.array([0.5, 0.7, 0.9, 1.2]))
    hyp = [(0, np.array([np.log(0.5), 0.1])), (1, np.append(la, 0.0)), (2, np.array([np.log(1.5), 0.0])),
           (3, np.append(la, 0.0)), (4, np.append(la, -0.1)), (5, np.array([np.log(0.6), 0.1])),
           (6, np.array([np.log(0.6), -0.1])), (7, np.append(la, 0.2)), (8, np.append(la, 0.0))]
    ln = np.log(0.3)
    means = [0.05 * i - 0.2 for i in range(9)]
    ptr = np.cumsum([0] + [r.size for r in rows])
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.concatenate(rows), list(range(9)), means)
    for k, (kind, h) in enumerate(hyp):
        ctx.set_hyper(k, kind, np.append(h, ln))
    mll, info, _ = ctx.fit()
    assert np.all(info == 0)
    g = ctx.gradients(D + 2)
    c2 = hipabi.Context(0)
    try:
        for l, (kind, h) in enumerate(hyp):
            ml = _single(c2, X[rows[l]], y[rows[l]], means[l], kind, h, ln)[0][0]
            gl = c2.gradients(D + 2)[0]
            assert abs(mll[l] - ml) <= 1e-12 * max(1.0, abs(ml)), l
            assert np.allclose(g[l], gl, rtol=1e-12, atol=1e-13 * max(1.0, np.max(np.abs(gl)))), l
            if kind >= 5:
                r = DenseGP(kind, dk.pack(kind, h[:-1], h[-1], logNoise=ln), X[rows[l]], y[rows[l]], means[l])
                go = r.grad()
                _ratio("nine kinds", np.abs(g[l][:go.size] - go), grad_tol(_cond(r), go))
                assert np.all(np.abs(g[l][:go.size] - go) <= grad_tol(_cond(r), go)), (l, g[l], go)
    finally:
        c2.close()


def _dense_leaves(m, X, y):
    return [DenseGP(lf.kernel.kind, dk.pack(lf.kernel.kind, lf.kernel.logl, lf.kernel.logs, logNoise=lf.logNoise), X[lf.obs], y[lf.obs], lf.mean.m)
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


@pytest.mark.parametrize("family,kind", [("dsmgp", 8), ("dsmgp", 5), ("dsmgp_depth4", 6), ("poe", 7), ("gpoe", 8),
                                         ("rbcm", 8), ("rbcm", 5)])
def test_whole_models_against_dense_leaves(family, kind):
    N, D = 3000, 4
    X, y, Xt = regression_data(N, D, n_test=200, seed=910)
    ll, ls, ln = (np.log([0.5, 0.7, 0.9, 1.2]) if is_ard(kind) else np.log(0.8)), 0.1, np.log(0.2)
    k = CLASSES[kind](ll, ls)
    mf = dsm.ConstMean(float(np.mean(y)))
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 3, 4, M=60, kernel=k, logNoise=ln, seed=4)
    elif family == "dsmgp_depth4":
        m = dsm.buildDSMGP(X, y, 2, 4, M=8, D=4, kernel=k, logNoise=ln, seed=9)
    elif family == "poe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=k, meanFun=mf, logNoise=ln, seed=4)
    elif family == "gpoe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=k, meanFun=mf, logNoise=ln, generalized=True, seed=4)
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
    elif family == "gpoe":
        mo, vo = ospn.predict_gpoe(m.root, gps, Xt)
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
    if is_ard(kind):
        assert m.leaves[0].kernel.dl.shape == (D,) and isinstance(m.leaves[0].kernel.ds, float)
    else:
        assert isinstance(m.leaves[0].kernel.dl, float) and isinstance(m.leaves[0].kernel.ds, float)


def test_mixed_kernel_vector_resident_test_rows_and_n_sub():
    N, D = 2000, 3
    X, y, Xt = regression_data(N, D, n_test=150, seed=930)
    kern = [dsm.IsoSE(np.log(0.4), 0.0), dsm.ArdMatern52(np.log([0.4, 0.6, 0.9]), 0.1)]
    kw = dict(M=60, logNoise=np.log(0.2), seed=5)
    m = dsm.buildDSMGP(X, y, 2, 4, kernel=kern, **kw)
    kinds = [lf.kernel.kind for lf in m.leaves]
    assert 0 in kinds and 8 in kinds
    c = hipabi.Context(0)
    try:
        for l in np.linspace(0, m.L - 1, 12).astype(int):
            lf = m.leaves[l]
            mll = _single(c, X[lf.obs], y[lf.obs], lf.mean.m, lf.kernel.kind, lf.kernel.loghyp(), lf.logNoise)[0][0]
            # a leaf of the model may continue a shared factor (PREFIX): other operation order than the leaf alone
            assert abs(m.leaf_mll[l] - mll) <= 1e-11 * max(1.0, abs(mll)), l
    finally:
        c.close()
    mu, var = dsm.predict(m, Xt)                               # the stand-alone prediction sweep
    # the test rows ride through the factorisation launches (build_factor_steps), predict only finishes them
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
    assert np.allclose(dsm.predict(m2, Xt)[0], mu, rtol=1e-11, atol=1e-13)
    dsm.updategradients(m)
    dsm.updategradients(m2)
    assert np.allclose(dsm.grad_mll(m), dsm.grad_mll(m2), rtol=1e-10, atol=1e-12)


def test_train_follows_a_dense_loop_and_irrelevant_dimensions_want_longer_lengthscales():
    N, D = 1500, 3
    X = uniform(77, 0, N * D).reshape((N, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.05 * normal(78, 0, N)          # only x_0 matters
    ll, ls, ln = np.log([0.3, 0.05, 0.05]), 0.0, np.log(0.1)
    kw = dict(M=200, logNoise=ln, seed=3)
    m = dsm.buildDSMGP(X, y, 2, 2, kernel=dsm.ArdMatern52(ll, ls), **kw)
    dsm.updategradients(m)
    g = dsm.grad_mll(m)
    assert g[1] > 0 and g[2] > 0                               # short length-scales on irrelevant inputs: grow them
    # three train! iterations against the same loop on dense leaves (grad_mll's tree weights from the device's leaf_mll)
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
    _, hist = dsm.train(m, dsm.ADAM(eta=0.05), iterations=3, randinit=False)
    out = dsm.getparams(m)
    assert np.allclose(out, ref, rtol=1e-9, atol=1e-12), (out, ref)
    assert np.all(out[1:D] > h[1:D])                           # the noise dimensions' length-scales moved up
    # an IsoMatern32 model trains as well: one length-scale, a scalar dl
    mi = dsm.buildDSMGP(X, y, 2, 2, kernel=dsm.IsoMatern32(np.log(0.3), 0.0), **kw)
    hi = dsm.getparams(mi).copy()
    dsm.train(mi, dsm.ADAM(eta=0.05), iterations=2, randinit=False)
    assert dsm.getparams(mi).size == 3 and np.all(dsm.getparams(mi) != hi)


@pytest.mark.parametrize("order", ["set_test_first", "hole_then_matern"])
def test_a_pooled_context_takes_its_kinds_after_set_test(order):
    """Under a device pool set_test builds the fused step lists at once: with no kernel id set yet (set_test_first), or with id 0
    still a hole while id 1 is set (hole_then_matern).  The Matern kind set afterwards -- and a later swap of which id is Matern --
    must still reach the diagonal blocks of its leaves.  40 leaves of 200 rows: both block steps run fused."""
    L, nl, D = 40, 200, 3
    X, y, Xt = _data(1700, L * nl, D, nt=60)
    nt = Xt.shape[0]
    rows = [np.arange(l * nl, (l + 1) * nl) for l in range(L)]
    ptr = np.cumsum([0] + [nl] * L)
    kid = [l % 2 for l in range(L)]
    means = [float(np.mean(y[r])) for r in rows]
    rptr, ridx = np.arange(L + 1) * nt, np.tile(np.arange(nt), L)
    ln = np.log(0.3)
    mat = np.append(np.log([0.5, 0.7, 0.9]), 0.1)
    se = np.array([np.log(0.4), 0.0])

    def reference(hyp):        # the same leaves in a plain context, the kinds set before anything else
        c = hipabi.Context(0)
        try:
            c.set_train(X, y)
            c.set_leaves(ptr, np.concatenate(rows), kid, means)
            for k, (kind, h) in hyp.items():
                c.set_hyper(k, kind, np.append(h, ln))
            c.set_test(Xt, rptr, ridx)
            mll, info, _ = c.fit()
            assert np.all(info == 0)
            c.predict_run()
            return (mll,) + c.predict_fetch()
        finally:
            c.close()

    ctx = hipabi.Context(0)
    try:
        ctx.reserve(1 << 30)
        ctx.set_train(X, y)
        ctx.set_leaves(ptr, np.concatenate(rows), kid, means)
        if order == "hole_then_matern":
            ctx.set_hyper(1, 0, np.append(se, ln))
        ctx.set_test(Xt, rptr, ridx)                           # pooled: the joint step lists are built here
        if order == "set_test_first":
            ctx.set_hyper(1, 0, np.append(se, ln))
        ctx.set_hyper(0, 8, np.append(mat, ln))
        for hyp in ({0: (8, mat), 1: (0, se)}, {0: (0, se), 1: (5, np.array([np.log(0.6), 0.2]))}):
            for k, (kind, h) in hyp.items():
                ctx.set_hyper(k, kind, np.append(h, ln))
            mll, info, _ = ctx.fit()
            assert np.all(info == 0)
            ctx.predict_run()
            mu, var = ctx.predict_fetch()
            rm, rmu, rvar = reference(hyp)
            assert np.allclose(mll, rm, rtol=1e-12, atol=0), float(np.max(np.abs(mll - rm)))
            assert np.allclose(mu, rmu, rtol=1e-10, atol=1e-12) and np.allclose(var, rvar, rtol=1e-10, atol=1e-12)
            for l in (0, 1, L - 2, L - 1):
                kind, h = hyp[kid[l]]
                if kind >= 5:
                    r = DenseGP(kind, dk.pack(kind, h[:-1], h[-1], logNoise=ln), X[rows[l]], y[rows[l]], means[l])
                    _ratio("pooled set_test", abs(mll[l] - r.mll()), mll_tol(r.mll(), _cond(r)))
                    assert abs(mll[l] - r.mll()) <= mll_tol(r.mll(), _cond(r)), l
    finally:
        ctx.close()
