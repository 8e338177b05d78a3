"""GPU tests of dsmgp_loo_gradients: the hyper-parameter gradients of every leaf's leave-one-out log predictive density (GPML
5.4.2, eq. 5.13) -- loo_weights_kernel, tile_ginv_kernel, loo_hvec_kernel, the LOO instantiations of the three tile_graddot
kernels and of ardlin_quad_kernel, and the host assembly.

References: tests/golden/gp_loo_grad.npz (50 digits, literal eq. 5.13; tests/golden/make_loo_grad_golden.py) for single leaves;
for leaf tables the float64 dense helper (tests/loo_grad_dense.py) on each leaf's downloaded factor; for the large and the
wide single GP central differences of the library's own lpd.  Tolerance: loo_grad_dense.tolerance, the project's gradient
rule."""
import os

import numpy as np
import pytest

from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd.datagen import uniform, normal
import dense_kernels as dk
import loo_grad_dense as lgd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = lgd.load_cases()
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}
SRC, CPY, PRE = 0, 32, 26       # the table's COPY leaf (of leaf 0) and its PREFIX leaf (of leaf 2)


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _single(ctx, X, y, mean, kind, hyp):
    """One leaf holding every row; hyp = the library hyper-vector including logNoise."""
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(mean)])
    ctx.set_hyper(0, int(kind), hyp)
    _, info, _ = ctx.fit()
    assert info[0] == 0


# ------------------------------------------------------------------------------------- (1) the 50-digit fixture

@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_against_50_digit_references(ctx, name):
    c = CASES[name]
    hyp = np.concatenate([c["loghyp"], [c["logNoise"]]])
    _single(ctx, c["X"], c["y"], c["mean"], c["kind"], hyp)
    g, lpd = ctx.loo_gradients(hyp.size)
    assert g.shape == (1, hyp.size) and lpd.shape == (1,)
    K = dk.value(c["kind"], c["loghyp"], c["X"], c["X"])
    tol = lgd.tolerance(c, c["grad"], K)
    err = np.abs(g[0] - c["grad"])
    print(f"\n{name}: cond {c['cond']:.3g} |g|inf {np.max(np.abs(c['grad'])):.3g} max err {np.max(err):.3g}, worst err/tol {np.max(err / tol):.3g}")
    assert np.all(err <= tol), (name, g[0], c["grad"], tol)
    assert _same_bits(lpd, ctx.loo()[2])
    g2, lpd2 = ctx.loo_gradients(hyp.size)
    assert _same_bits(g, g2) and _same_bits(lpd, lpd2)
    if c["kind"] in (2, 3):
        assert g[0, -2] == 0.0          # the dummy variance slot


# ------------------------------------------------------------------------------------- (2) the leaf table

def _table_setup(ctx, mean=None):
    T = TABLE
    ctx.set_train(T["X"], T["y"])
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean"] if mean is None else mean)
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])


def _table_check(ctx, tag, mean, g, factor=2.0):
    """Every leaf against the dense helper on its downloaded factor and kernel_matrix; twice the tolerance (both sides round)."""
    T = TABLE
    op_, ob = T["obs_ptr"], T["obs_idx"]
    worst = 0.0
    for l in range(T["kid"].size):
        a, b = int(op_[l]), int(op_[l + 1])
        rows = ob[a:b]
        kid = int(T["kid"][l])
        kind = int(T["kinds"][kid])
        hyp = T["hyp"][kid][:T["hyp_len"][kid]]
        noise = float(np.exp(2.0 * hyp[-1]))
        F, _ = ctx.download_factor(l, b - a)
        F = np.tril(F)
        Xl = np.asfortranarray(T["X"][rows])
        ref = lgd.loo_grad_from_factor(F, dk.d_hyper(kind, hyp[:-1], Xl)[1], noise, T["y"][rows], float(mean[l]))
        sv = np.linalg.svd(F, compute_uv=False)
        case = dict(kind=kind, cond=float((sv[0] / sv[-1]) ** 2), weak=False, logNoise=float(hyp[-1]))
        tol = factor * lgd.tolerance(case, ref)
        r = float(np.max(np.abs(g[l, :ref.size] - ref) / tol))
        assert r <= 1.0, (tag, l, kind, g[l, :ref.size], ref, tol)
        assert np.all(g[l, ref.size:] == 0.0)
        worst = max(worst, r)
    print(f"\n{tag}: {T['kid'].size} leaves, worst err/tol {worst:.3g}")


def test_leaf_table_lanes_and_step_kinds(ctx):
    """The 41-leaf table of gp_pred.npz (FULL, COPY and PREFIX leaves, several kinds in one context) with DSMGP_OPT_LANES 1 and 2
    and DSMGP_OPT_FUSED_STEPS 0 and 1; the COPY leaf with its source's mean equals its source, with another mean it does not."""
    T = TABLE
    stride = int(np.max(T["hyp_len"]))
    try:
        for lanes, fused in ((1, 1), (2, 1), (1, 0), (2, 0)):
            ctx.set_option(hipabi.OPT_FUSED_STEPS, fused)
            ctx.set_option(hipabi.OPT_LANES, lanes)
            _table_setup(ctx)
            _, info, _ = ctx.fit()
            assert np.all(info == 0)
            g, lpd = ctx.loo_gradients(stride)
            assert _same_bits(lpd, ctx.loo()[2])
            assert _same_bits(g[CPY], g[SRC])
            _table_check(ctx, f"table lanes={lanes} fused_steps={fused}", T["mean"], g)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)
    mean2 = T["mean"].copy()
    mean2[CPY] += 0.25
    _table_setup(ctx, mean2)
    ctx.fit()
    g2, _ = ctx.loo_gradients(stride)
    assert not _same_bits(g2[CPY], g2[SRC])
    _table_check(ctx, "table, COPY leaf with another mean", mean2, g2)


# ------------------------------------------------------------------------------------- (3) large and wide single GPs

def _fd_lpd(ctx, X, y, mean, kind, hyp, j, e=1e-5):
    out = []
    for s in (+1.0, -1.0):
        h = hyp.copy()
        h[j] += s * e
        _single(ctx, X, y, mean, kind, h)
        out.append(ctx.loo()[2][0])
    return (out[0] - out[1]) / (2 * e)


@pytest.mark.parametrize("n,D", [(3000, 4), (700, 40)])
def test_single_gp_against_central_differences_of_lpd(ctx, n, D):
    """n = 3000: 24 row tiles, the last one ragged (56 rows); D = 40 > GRADDOT_STAGE_D: the global-memory branch of the IsoSE
    epilogue.  Central differences of ctx.loo()'s lpd, 2e-6 max(1, |fd|) as the existing finite-difference tests."""
    X = uniform(9000 + n + D, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) + np.cos(2.0 * X[:, 1]) + 0.1 * normal(9100 + n + D, 0, n)
    mean = float(np.mean(y)) + 0.2
    hyp = np.array([np.log(0.3 * np.sqrt(D)), 0.1, np.log(0.2)])
    _single(ctx, X, y, mean, 0, hyp)
    g, _ = ctx.loo_gradients(3)
    for j in range(3):
        fd = _fd_lpd(ctx, X, y, mean, 0, hyp, j)
        print(f"\nn={n} D={D} component {j}: {g[0, j]:.10g} fd {fd:.10g}")
        assert abs(g[0, j] - fd) <= 2e-6 * max(1.0, abs(fd)), (j, g[0, j], fd)


# ------------------------------------------------------------------------------------- (4) non-interference

def test_gradients_and_loo_unchanged_and_call_orders_agree(ctx):
    T = TABLE
    L = T["kid"].size
    stride = int(np.max(T["hyp_len"]))
    _table_setup(ctx)
    ctx.fit()
    first = ctx.loo_gradients(stride)                      # loo_gradients first
    ctx.fit()
    loo0 = ctx.loo()
    after_loo = ctx.loo_gradients(stride)                  # after loo
    ctx.fit()
    g0 = ctx.gradients(stride)
    after_grad = ctx.loo_gradients(stride)                 # after gradients
    for other in (after_loo, after_grad):
        assert _same_bits(first[0], other[0]) and _same_bits(first[1], other[1])
    assert _same_bits(g0, ctx.gradients(stride))
    assert all(_same_bits(p, q) for p, q in zip(loo0, ctx.loo()))
    mask = np.zeros(L, dtype=np.int32)
    mask[[3, 7, CPY]] = 1                                  # leaves owners out
    try:
        ctx.set_gradient_leaves(mask)
        ctx.fit()
        gm = ctx.gradients(stride)
        masked = ctx.loo_gradients(stride)                 # the mask does not apply
        assert _same_bits(first[0], masked[0]) and _same_bits(first[1], masked[1])
        assert _same_bits(gm, ctx.gradients(stride))
        assert all(_same_bits(p, q) for p, q in zip(loo0, ctx.loo()))
    finally:
        ctx.set_gradient_leaves(None)
    assert _same_bits(g0, ctx.gradients(stride))


# ------------------------------------------------------------------------------------- (5) failures and errors

def test_failed_leaf_gets_nan_and_the_others_keep_their_bits(ctx):
    n0, n1 = 140, 100
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    hyp1 = np.array([np.log(0.3), 0.0, np.log(0.1)])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, hyp1)
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    g, lpd = ctx.loo_gradients(3)
    assert np.all(np.isnan(g[0])) and np.isnan(lpd[0]) and np.all(np.isfinite(g[1]))
    _single(ctx, np.asfortranarray(X[n0:]), y[n0:], 0.2, 0, hyp1)
    alone, lpd1 = ctx.loo_gradients(3)
    assert _same_bits(g[1], alone[0]) and _same_bits(lpd[1:], lpd1)


def test_errors_leave_a_usable_context():
    c = hipabi.Context(0)
    try:
        X = uniform(9300, 0, 200).reshape((100, 2), order="F")
        y = np.sin(3.0 * X[:, 0])
        c.set_train(X, y)
        c.set_leaves([0, 100], np.arange(100), [0], [0.1])
        c.set_hyper(0, 0, [np.log(0.3), 0.0, np.log(0.1)])
        with pytest.raises(hipabi.DsmgpError) as ei:
            c.loo_gradients(3)
        assert ei.value.code == hipabi.E_STATE
        c.fit()
        with pytest.raises(hipabi.DsmgpError) as ei:
            c.loo_gradients(2)
        assert ei.value.code == hipabi.E_ARG
        g, lpd = c.loo_gradients(3)
        assert np.all(np.isfinite(g)) and _same_bits(lpd, c.loo()[2])
    finally:
        c.close()


# ------------------------------------------------------------------------------------- (6) model level

def test_model_grad_loo_train_and_default_path():
    import deepstructuredmixtures_amd as dsm
    from deepstructuredmixtures_amd.datagen import regression_data
    X, y, _ = regression_data(600, 2, n_test=1, seed=9400)

    def build():
        return dsm.buildDSMGP(X, y, 2, 2, M=60, D=2, kernel=dsm.IsoSE(np.log(0.5), 0.0), meanFun=dsm.ConstMean(float(np.mean(y))),
                              logNoise=np.log(0.3))

    m = build()
    dsm.fit(m)
    dsm.updategradients(m, objective="loo")
    g = dsm.grad_loo(m)
    h0 = dsm.getparams(m).copy()
    assert g.size == h0.size
    for j in range(h0.size):
        v = []
        for s in (+1.0, -1.0):
            h = h0.copy()
            h[j] += s * 1e-5
            dsm.setparams(m, h)
            dsm.fit(m)
            v.append(dsm.loo_objective(m))
        fd = (v[0] - v[1]) / 2e-5
        print(f"\nmodel component {j}: grad_loo {g[j]:.10g} fd {fd:.10g}")
        assert abs(g[j] - fd) <= 2e-6 * max(1.0, abs(fd)), (j, g[j], fd)
    dsm.setparams(m, h0)
    m, hist = dsm.train(m, dsm.ADAM(eta=0.01), objective="loo", randinit=False, iterations=20)
    dsm.fit(m)
    assert hist.size == 20 and dsm.loo_objective(m) > hist[0]
    a, ha = dsm.train(build(), randinit=False, iterations=5)
    b, hb = dsm.train(build(), randinit=False, iterations=5, objective="mll")
    assert _same_bits(ha, hb) and _same_bits(dsm.getparams(a), dsm.getparams(b))
    with pytest.raises(ValueError):
        dsm.train(build(), objective="elbo", iterations=1)
