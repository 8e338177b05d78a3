"""GPU suite for the ArdSEProduct kernel (DSMGP_KIND_ARD_SE_PRODUCT): Gram tiles, single leaves and gradients against the
50-digit references of tests/golden/gp_ardse_product.npz, the IsoSE identity at equal length-scales, gradients by central
differences at D up to 48, mixed kernel vectors, whole models against the dense restatement of tests/dense_gp.py,
train! and the refusals.  Tolerances come from tests/pred_tolerance.py (mll_tol, moment_tol) and the gradient fixture's rule
64 cond_2(K_y) eps max(1, |g|_inf) (tests/test_gradients_gpu.py)."""
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


def dense_z(logl, x1, x2):
    """The exponent z = -sum_d (a_d - b_d)^2 / (2 l_d^2)."""
    return -0.5 * dk.scaled_sqdist(4, dk.pack(4, logl), x1, x2)


KIND = dsm.kernels.KIND_ARD_SE_PRODUCT
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_ardse_product.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files})
WORST = {}


def _case(name):
    return {k.split("/")[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}


def _ratio(group, err, tol):
    r = float(np.max(np.asarray(err) / np.asarray(tol)))
    WORST[group] = max(WORST.get(group, 0.0), r)
    print(f"\n[{group}] worst err/tol {WORST[group]:.3g}")
    return r


def grad_tol(cond, ref):
    return max(1e-13, 64.0 * float(cond) * EPS * max(1.0, float(np.max(np.abs(ref)))))


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _data(seed, n, D, nt=100):
    X = uniform(seed, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3 * X[:, 0]) + 0.3 * X[:, -1] + 0.1 * normal(seed + 1, 0, n)
    Xt = uniform(seed + 2, 0, nt * D).reshape((nt, D), order="F")
    return X, y, Xt


def _logl(D):
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


@pytest.mark.parametrize("D", [1, 3, 8, 32, 33, 48])
def test_kernel_matrix_against_the_dense_formula(ctx, D):
    n1, n2 = 300, 131
    x1 = uniform(500 + D, 0, n1 * D).reshape((n1, D), order="F")
    x2 = uniform(600 + D, 0, n2 * D).reshape((n2, D), order="F")
    ll, ls = _logl(D), 0.2
    ctx.set_train(x1, np.zeros(n1))
    ctx.set_hyper(0, KIND, list(ll) + [ls, 0.0])
    K = ctx.kernel_matrix(0, x1, x2)
    Kd = dk.value(4, dk.pack(4, ll, ls), x1, x2)
    # both sides round z = sum_d u_d^2 nh_d in D steps (|dz| <= (D + 2) eps |z|), then exp and the sigma^2 product
    tol = Kd * (2 * (D + 2) * EPS * np.abs(dense_z(ll, x1, x2)) + 8 * EPS) + 1e-300
    _ratio("gram", np.abs(K - Kd), tol)
    assert np.all(np.abs(K - Kd) <= tol)
    Ks = ctx.kernel_matrix(0, x1, x1)
    assert np.array_equal(Ks, Ks.T)                            # bit-symmetric


@pytest.mark.parametrize("name", CASES)
def test_single_leaf_against_50_digit_references(ctx, name):
    c = _case(name)
    X, y, Xt = c["X"], c["y"], c["Xt"]
    D = X.shape[1]
    h = np.append(c["logl"], float(c["logs"]))
    m = min(X.shape[0], 8)
    ctx.set_train(X, y)
    ctx.set_hyper(0, KIND, np.append(h, float(c["logNoise"])))
    Kc = ctx.kernel_matrix(0, X[:m], X[:m])
    Kt = ctx.kernel_matrix(0, X[:m], Xt)
    zc = dense_z(c["logl"], X[:m], X[:m])
    tolK = np.abs(c["Kc"]) * (2 * (D + 2) * EPS * np.abs(zc) + 8 * EPS)
    _ratio("golden K", np.abs(Kc - c["Kc"]), tolK + 1e-300)
    assert np.all(np.abs(Kc - c["Kc"]) <= tolK + 1e-300)
    tolT = np.abs(c["Kt"]) * (2 * (D + 2) * EPS * np.abs(dense_z(c["logl"], X[:m], Xt)) + 8 * EPS)
    assert np.all(np.abs(Kt - c["Kt"]) <= tolT + 1e-300)
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
            mll, info, _ = _single(ctx, X, y, float(c["mean"]), KIND, h, float(c["logNoise"]))
            assert info[0] == 0
            _ratio("golden mll", abs(mll[0] - c["mll"]), tml)
            assert abs(mll[0] - c["mll"]) <= tml, (fg, fs, lanes, mll[0], float(c["mll"]))
            mu, var = ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
            _ratio("golden moments", np.concatenate([np.abs(mu - c["mu"]) / tmu, np.abs(var - c["var"]) / tvar]), 1.0)
            assert np.all(np.abs(mu - c["mu"]) <= tmu) and np.all(np.abs(var - c["var"]) <= tvar), (fg, fs, lanes)
            g = ctx.gradients(D + 2)[0]
            _ratio("golden gradients", np.abs(g - c["grad"]), tg)
            assert np.all(np.abs(g - c["grad"]) <= tg), (fg, fs, lanes, g, c["grad"])
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)


@pytest.mark.parametrize("n,D", [(515, 3), (1300, 8), (400, 36)])
def test_equal_lengthscales_are_iso_se(ctx, n, D):
    """ArdSEProduct(l, ..., l; s) = IsoSE(l; s) in mll and moments; sum_d dl_d * sigma = IsoSE's dl and ds * sigma = IsoSE's ds
    (the reference's factor sigma on IsoSE); dnoise equal."""
    X, y, Xt = _data(900 + n, n, D)
    ln, mean, l0, ls = np.log(0.3), float(np.mean(y)), np.log(0.4 * np.sqrt(D)), 0.3
    ma = _single(ctx, X, y, mean, KIND, np.append(np.full(D, l0), ls), ln)[0][0]
    mua, vara = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    ga = ctx.gradients(D + 2)[0]
    mi = _single(ctx, X, y, mean, 0, np.array([l0, ls]), ln)[0][0]
    mui, vari = ctx.predict_leaves(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    gi = ctx.gradients(3)[0]
    g = DenseGP(4, dk.pack(4, np.full(D, l0), ls, logNoise=ln), X, y, mean)
    cond = _cond(g)
    assert abs(ma - mi) <= mll_tol(mi, cond)
    _ratio("iso identity", abs(ma - mi), mll_tol(mi, cond))
    tmu, tvar = moment_tol(mui, vari, np.exp(2 * ls), np.exp(2 * ln), max(1.0, np.max(np.abs(y))))
    assert np.all(np.abs(mua - mui) <= tmu) and np.all(np.abs(vara - vari) <= tvar)
    sigma = np.exp(ls)
    iso = np.array([np.sum(ga[:D]) * sigma, ga[D] * sigma, ga[D + 1]])
    tg = grad_tol(cond, gi)
    _ratio("iso identity", np.abs(iso - gi), tg)
    assert np.all(np.abs(iso - gi) <= tg), (iso, gi)


@pytest.mark.parametrize("D", [1, 8, 35, 36, 48])
def test_gradients_against_the_dense_trace_and_finite_differences(ctx, D):
    n = 300
    X, y, _ = _data(1100 + D, n, D, nt=4)
    ll, ls, ln, mean = _logl(D), 0.1, np.log(0.25), float(np.mean(y))
    h = np.append(ll, ls)
    _single(ctx, X, y, mean, KIND, h, ln)
    g = ctx.gradients(D + 2)[0]
    dg = DenseGP(4, dk.pack(4, ll, ls, logNoise=ln), X, y, mean)
    go = dg.grad()
    tg = grad_tol(_cond(dg), go)
    _ratio("gradients dense", np.abs(g - go), tg)
    assert np.all(np.abs(g - go) <= tg), (g, go)
    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
    try:
        if D <= 35:
            _single(ctx, X, y, mean, KIND, h, ln)
            assert np.array_equal(ctx.gradients(D + 2)[0], g)       # the ArdSE option does not touch ArdSEProduct
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    eps = 1e-5
    full = np.append(h, ln)
    for j in sorted(set([0, D // 2, D - 1, D, D + 1])):
        hp, hm = full.copy(), full.copy()
        hp[j] += eps
        hm[j] -= eps
        fd = (_single(ctx, X, y, mean, KIND, hp[:-1], hp[-1])[0][0] - _single(ctx, X, y, mean, KIND, hm[:-1], hm[-1])[0][0]) / (2 * eps)
        # central difference: truncation eps^2 |f'''| plus rounding 64 cond eps |mll| / eps
        tol = 1e-6 * max(1.0, abs(fd)) + 64 * _cond(dg) * EPS * max(1.0, abs(dg.mll())) / eps
        _ratio("finite differences", abs(g[j] - fd), tol)
        assert abs(g[j] - fd) <= tol, (j, g[j], fd)


def test_gradients_on_copy_and_prefix_leaves_and_under_a_leaf_mask(ctx):
    """Leaf 0 (300 rows), leaf 1 = COPY of it (same mean: shares its sums), leaf 2 = COPY with a mean of its own, leaf 3 =
    PREFIX: 600 rows whose first 300 are leaf 0's (factor continued from column 300)."""
    n, D = 600, 5
    X, y, _ = _data(1400, n, D, nt=4)
    ll, ls, ln = _logl(D), 0.0, np.log(0.3)
    means = [0.1, 0.1, -0.4, 0.2]
    rows = [np.arange(300), np.arange(300), np.arange(300), np.arange(n)]
    ptr = np.cumsum([0] + [r.size for r in rows])
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.concatenate(rows), [0, 0, 0, 0], means)
    ctx.set_hyper(0, KIND, np.concatenate([ll, [ls, ln]]))
    ctx.set_sharing([0, 1, 1, 2], [-1, 0, 0, 0], [0, 0, 0, 300])
    mll, info, _ = ctx.fit()
    assert np.all(info == 0)
    g = ctx.gradients(D + 2)
    for l in range(4):
        r = DenseGP(4, dk.pack(4, ll, ls, logNoise=ln), X[rows[l]], y[rows[l]], means[l])
        cond = _cond(r)
        assert abs(mll[l] - r.mll()) <= mll_tol(r.mll(), cond)
        go = r.grad()
        _ratio("copy/prefix/mask", np.abs(g[l] - go), grad_tol(cond, go))
        assert np.all(np.abs(g[l] - go) <= grad_tol(cond, go)), (l, g[l], go)
    assert np.array_equal(g[0], g[1])                          # copygradients
    for mask in ([0, 1, 0, 1], [0, 0, 1, 0], [1, 0, 0, 0]):
        ctx.set_gradient_leaves(mask)
        gm = ctx.gradients(D + 2)
        for l in range(4):
            if mask[l]:     # another task list: the per-task sums are added in another order
                assert np.allclose(gm[l], g[l], rtol=1e-12, atol=1e-14 * np.max(np.abs(g[l]))), (mask, l)
            else:
                assert np.all(gm[l] == 0.0)
    ctx.set_gradient_leaves(None)


def test_refusals_leave_a_usable_context(ctx):
    n, D = 200, 3
    X, y, _ = _data(1500, n, D, nt=4)
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
    for bad in ([0.1, 0.2, 0.0, np.log(0.3)], [0.1, 0.2, 0.3, 0.4, 0.0, np.log(0.3)]):   # D - 1 and D + 1 length-scales
        with pytest.raises(hipabi.DsmgpError) as e:
            ctx.set_hyper(0, KIND, bad)
        assert e.value.code == -1                               # DSMGP_E_ARG
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.set_hyper(0, 5, [0.1, 0.2, 0.3, 0.0, np.log(0.3)])
    assert e.value.code == -1
    ctx.set_hyper(0, KIND, [0.1, 0.2, 0.3, 0.0, np.log(0.3)])
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    r = DenseGP(4, dk.pack(4, [0.1, 0.2, 0.3], 0.0, logNoise=np.log(0.3)), X, y, 0.0)
    assert abs(mll[0] - r.mll()) <= mll_tol(r.mll(), _cond(r))


def test_one_context_with_every_kind_equals_each_leaf_alone(ctx):
    """IsoSE, ArdSEProduct and ArdLinear leaves side by side in one context (kernel ids 0, 1, 2)."""
    D = 4
    X, y, _ = _data(1600, 900, D, nt=4)
    rows = [np.arange(0, 300), np.arange(300, 650), np.arange(650, 900)]
    hyp = [(0, np.array([np.log(0.5), 0.1])), (KIND, np.append(_logl(D), -0.1)), (3, np.append(_logl(D), 0.0))]
    ln = np.log(0.3)
    ptr = np.cumsum([0] + [r.size for r in rows])
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.concatenate(rows), [0, 1, 2], [0.0, 0.1, -0.1])
    for k, (kind, h) in enumerate(hyp):
        ctx.set_hyper(k, kind, np.append(h, ln))
    mll, info, _ = ctx.fit()
    g = ctx.gradients(D + 2)
    c2 = hipabi.Context(0)
    try:
        for l, (kind, h) in enumerate(hyp):
            ml = _single(c2, X[rows[l]], y[rows[l]], [0.0, 0.1, -0.1][l], kind, h, ln)[0][0]
            gl = c2.gradients(D + 2)[0]
            assert abs(mll[l] - ml) <= 1e-12 * max(1.0, abs(ml)), l
            assert np.allclose(g[l], gl, rtol=1e-12, atol=1e-13 * max(1.0, np.max(np.abs(gl)))), l
    finally:
        c2.close()


def _dense_leaves(m, X, y):
    return [DenseGP(4, dk.pack(4, lf.kernel.logl, lf.kernel.logs, logNoise=lf.logNoise), X[lf.obs], y[lf.obs], lf.mean.m) for lf in ptree.get_leaves(m.root)]


def _rbcm(root, gps, x, s):
    C = 1.0 / s
    mu = np.zeros(x.shape[0])
    for c in root.children:
        m_, t_ = ospn._predict_poe(c, gps, x)
        beta = 0.5 * (np.log(s) - np.log(1.0 / t_))
        C = C + beta * t_ - beta / s
        mu = mu + m_ * (beta * t_)
    return mu / C, 1.0 / C


@pytest.mark.parametrize("family", ["dsmgp", "dsmgp_depth4", "poe", "gpoe", "rbcm"])
def test_whole_models_against_dense_leaves(family):
    N, D = 3000, 4
    X, y, Xt = regression_data(N, D, n_test=200, seed=910)
    ll, ls, ln = np.log([0.5, 0.7, 0.9, 1.2]), 0.1, np.log(0.2)
    k = dsm.ArdSEProduct(ll, ls)
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
    else:
        mo, vo = _rbcm(m.root, gps, Xt, np.full(Xt.shape[0], np.exp(2 * ls) + np.exp(2 * ln)))
    # leaf moments within 64 cond eps; the aggregate carries them (the north-star RTOL bounds both)
    tmu, tvar = moment_tol(mo, vo, np.exp(2 * ls), np.exp(2 * ln), max(1.0, np.max(np.abs(y))))
    _ratio("whole models", np.concatenate([np.abs(mu - mo) / tmu, np.abs(var - vo) / tvar]), 1.0)
    assert np.all(np.abs(mu - mo) <= tmu) and np.all(np.abs(var - vo) <= tvar)
    g = dsm.updategradients(m).copy()
    for l, r in enumerate(gps):
        go = r.grad()
        assert np.all(np.abs(g[l, :D + 2] - go) <= grad_tol(conds[l], go)), l
    assert m.leaves[0].kernel.dl.shape == (D,) and isinstance(m.leaves[0].kernel.ds, float)


def test_mixed_kernel_vector_and_parameters():
    N, D = 2000, 3
    X, y, Xt = regression_data(N, D, n_test=100, seed=930)
    kern = [dsm.IsoSE(np.log(0.4), 0.0), dsm.ArdSEProduct(np.log([0.4, 0.6, 0.9]), 0.1)]
    m = dsm.buildDSMGP(X, y, 2, 4, M=60, kernel=kern, logNoise=np.log(0.2), seed=5)
    kinds = [lf.kernel.kind for lf in m.leaves]
    assert 0 in kinds and KIND in kinds
    c = hipabi.Context(0)
    try:
        for l in np.linspace(0, m.L - 1, 12).astype(int):
            lf = m.leaves[l]
            mll = _single(c, X[lf.obs], y[lf.obs], lf.mean.m, lf.kernel.kind, lf.kernel.loghyp(), lf.logNoise)[0][0]
            assert abs(m.leaf_mll[l] - mll) <= 1e-12 * max(1.0, abs(mll)), l
    finally:
        c.close()
    p = dsm.getparams(m)
    dsm.setparams(m, p)
    assert np.array_equal(dsm.getparams(m), p)


def test_train_follows_a_dense_loop_and_irrelevant_dimensions_want_longer_lengthscales():
    N, D = 1500, 3
    X = uniform(77, 0, N * D).reshape((N, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.05 * normal(78, 0, N)          # only x_0 matters
    ll, ls, ln = np.log([0.3, 0.05, 0.05]), 0.0, np.log(0.1)
    kw = dict(M=200, logNoise=ln, seed=3)
    m = dsm.buildDSMGP(X, y, 2, 2, kernel=dsm.ArdSEProduct(ll, ls), **kw)
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
        for lf, r in zip(m.leaves, gps):
            assert abs(m.leaf_mll[m.leaves.index(lf)] - r.mll()) <= mll_tol(r.mll(), _cond(r))
        m.leaf_grad = np.array([r.grad() for r in gps])
        ref = ref + opt.apply(ref, dsm.grad_mll(m))
    dsm.setparams(m, h)
    dsm.fit(m)
    _, hist = dsm.train(m, dsm.ADAM(eta=0.05), iterations=3, randinit=False)
    out = dsm.getparams(m)
    assert np.allclose(out, ref, rtol=1e-9, atol=1e-12), (out, ref)
    assert np.all(out[:D] != h[:D])
