"""GPU tests of dsmgp_solve_targets / dsmgp_predict_targets / dsmgp_targets_fetch: several target columns on one
factorisation, through hipabi.Context and the model API (fit_targets / predict_targets).

References: tests/golden/gp_targets.npz (50 digits, tests/golden/make_targets_golden.py) for single leaves; for the sweep's
shapes and the leaf table a float64 reference formed by tests/targets_dense.py from download_factor / kernel_matrix of the same
context -- twice the tolerance there, both sides round.  Tolerances: targets_dense.z_tol / mll_tol (condition of the factor)
and mu_tol (pred_tolerance.moment_tol); the model API at pred_tolerance.agg_tol."""
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import targets_dense as td
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel
from pred_tolerance import agg_tol, moment_tol, row_entries

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = td.load_cases()
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}
SRC, CPY, PRE = 0, 32, 26       # the table's COPY leaf (of leaf 0) and its PREFIX leaf (of leaf 2)


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check(tag, got, ref, tol):
    """Every element within its tolerance; prints the worst error and error / tolerance."""
    got, ref = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, ref))
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = np.abs(got - ref)
    ratio = err / tol
    worst = int(np.argmax(ratio)) if ratio.size else 0
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    assert np.all(err <= tol), (tag, worst, got.flat[worst], ref.flat[worst], tol.flat[worst])
    return float(np.max(ratio))


def _single(ctx, X, y, mean, kind, loghyp, logNoise, Xt=None):
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(mean)])
    ctx.set_hyper(0, int(kind), np.concatenate([loghyp, [float(logNoise)]]))
    if Xt is not None:
        ctx.set_test(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    return mll


def _columns(seed, X, Q):
    """Q target columns over the rows of X: smooth functions of the inputs with offsets and noise of different sizes."""
    rng = np.random.default_rng(seed)
    n = X.shape[0]
    j = np.arange(Q)
    return (np.sin((1.0 + j)[None, :] * X[:, :1]) * (1.0 + j)[None, :] + 10.0 * (j % 3)[None, :]
            + 0.1 * rng.standard_normal((n, Q)))


# ------------------------------------------------------------------------------------- (1) fixture cases

@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_against_50_digit_references(ctx, name):
    c = CASES[name]
    n = c["X"].shape[0]
    _single(ctx, c["X"], c["Y"][:, 0], c["mean"][0], c["kind"], c["loghyp"], c["logNoise"], Xt=c["Xt"])
    mll, _ = ctx.solve_targets(c["Y"], c["mean"][None, :])
    ctx.predict_run()
    mu = ctx.predict_targets()
    Z = ctx.targets_fetch(0)
    assert Z.shape == (n, 3) and mll.shape == (1, 3) and mu.shape == (c["Xt"].shape[0], 3)
    F, _ = ctx.download_factor(0, n)
    _check(name + " Z", Z, c["Z"], td.z_tol(c["Z"], c["cond"]))
    _check(name + " mll", mll[0], c["mll"], td.mll_tol(c["Z"], F, c["cond"]))
    _check(name + " mu", mu, c["mu"], td.mu_tol(c["mu"], c["Y"]))


# ------------------------------------------------------------------------------------- (2) shapes of the sweep

_DENSE = {}


def _dense_leaf(ctx, leaf, kid, Xl, Yl, mean, Xt_rows):
    """(Z, mll, mu, cond, F) of one leaf from the context's own factor and kernel matrix."""
    n = Xl.shape[0]
    F, _ = ctx.download_factor(leaf, n)
    Ktn = ctx.kernel_matrix(kid, np.asfortranarray(Xt_rows), np.asfortranarray(Xl)) if Xt_rows is not None else None
    Z, mll, mu = td.reference(F, Yl, mean, Ktn)
    return Z, mll, mu, td.factor_cond(F), F


@pytest.mark.parametrize("n", [1, 100, 128, 129, 300])
def test_sweep_shapes_against_the_dense_reference(ctx, n):
    """One partial block, one full block, a second block of one row, three blocks; Q on both sides of the MFMA width; one test
    row and two row tiles of test rows.  One fit per n, every (Q, n_t) on it."""
    D = 2
    rng = np.random.default_rng(100 + n)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    hyp, logNoise = np.array([np.log(0.4), 0.1]), np.log(0.1)
    Yall = _columns(n, X, 17)
    for nt in (1, 130):
        Xt = np.asfortranarray(rng.uniform(size=(nt, D)) * 1.2 - 0.1)
        _single(ctx, X, Yall[:, 0], 0.0, 0, hyp, logNoise, Xt=Xt)
        ctx.predict_run()
        for Q in (1, 3, 16, 17):
            Y = Yall[:, :Q]
            mean = np.mean(Y, axis=0)
            mll, _ = ctx.solve_targets(Y, mean[None, :])
            mu = ctx.predict_targets()
            Z = ctx.targets_fetch(0)
            rZ, rmll, rmu, cond, F = _dense_leaf(ctx, 0, 0, X, Y, mean, Xt)
            tag = f"n {n} nt {nt} Q {Q}"
            _check(tag + " Z", Z, rZ, 2.0 * td.z_tol(rZ, cond))
            _check(tag + " mll", mll[0], rmll, 2.0 * td.mll_tol(rZ, F, cond))
            _check(tag + " mu", mu, rmu, 2.0 * td.mu_tol(rmu, Y))


# ------------------------------------------------------------------------------------- (3) the leaf table

def _table_setup(ctx, lanes=0, joint=True):
    T = TABLE
    ctx.set_option(hipabi.OPT_LANES, lanes)
    ctx.set_joint(joint)
    ctx.set_train(T["X"], T["y"])
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean"])
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])
    ctx.set_test(T["Xt"], T["route_ptr"], T["route_idx"])


def _table_targets(Q=3):
    """Targets over the table's training rows and a mean per (leaf, column): COPY and PREFIX leaves with means of their own."""
    T = TABLE
    Y = np.concatenate([T["y"][:, None], _columns(7, T["X"], Q - 1)], axis=1)
    L = T["kid"].size
    mean = np.stack([np.mean(Y[T["obs_idx"][int(T["obs_ptr"][l]):int(T["obs_ptr"][l + 1])]], axis=0) for l in range(L)])
    mean[:, 0] = T["mean"]
    mean[CPY, 1:] += 0.37
    mean[PRE, 1:] -= 0.21
    return Y, mean


def _table_run(ctx, Y, mean):
    _, info, _ = ctx.fit()
    assert np.all(info == 0)
    ctx.predict_run()
    mll, _ = ctx.solve_targets(Y, mean)
    mu = ctx.predict_targets()
    Z = [ctx.targets_fetch(l) for l in range(TABLE["kid"].size)]
    return mll, mu, Z


def _table_reference(ctx, Y, mean):
    key = "table"
    if key not in _DENSE:
        T = TABLE
        ref = []
        for l in range(T["kid"].size):
            a, b = int(T["obs_ptr"][l]), int(T["obs_ptr"][l + 1])
            rows = T["obs_idx"][a:b]
            ra, rb = int(T["route_ptr"][l]), int(T["route_ptr"][l + 1])
            xt = T["Xt"][T["route_idx"][ra:rb]] if rb > ra else None
            ref.append(_dense_leaf(ctx, l, int(T["kid"][l]), T["X"][rows], Y[rows], mean[l], xt))
        _DENSE[key] = ref
    return _DENSE[key]


def _table_check(tag, T, ref, mll, mu, Z, Y, factor=2.0):
    worst = 0.0
    for l, (rZ, rmll, rmu, cond, F) in enumerate(ref):
        rows = T["obs_idx"][int(T["obs_ptr"][l]):int(T["obs_ptr"][l + 1])]
        r = [np.max(np.abs(Z[l] - rZ) / (factor * td.z_tol(rZ, cond))),
             np.max(np.abs(mll[l] - rmll) / (factor * td.mll_tol(rZ, F, cond)))]
        if rmu is not None:
            ra, rb = int(T["route_ptr"][l]), int(T["route_ptr"][l + 1])
            r.append(np.max(np.abs(mu[ra:rb] - rmu) / (factor * td.mu_tol(rmu, Y[rows]))))
        assert max(r) <= 1.0, (tag, l, r)
        worst = max(worst, float(max(r)))
    print(f"\n{tag}: {len(ref)} leaves, worst err/tol {worst:.3g}")


def _factors(ctx):
    T = TABLE
    return [np.tril(ctx.download_factor(l, int(T["obs_ptr"][l + 1] - T["obs_ptr"][l]))[0]) for l in range(T["kid"].size)]


def test_leaf_table_lanes_and_routes(ctx):
    """The 41-leaf table of gp_pred.npz with its COPY and its PREFIX leaf, targets and means of their own: every leaf against
    the dense reference on both routes to K_tn L^-T (rows through the fit, standalone sweep) and with one lane and two; mu of the
    two routes within tolerance of each other.
    One lane against two on bits: OPT_LANES rebuilds the plan, and the FIT's factors under two lanes agree with one lane's to
    rounding only (include/dsmgp_hip.h at DSMGP_OPT_LANES: a launch of half the tiles cuts its tail along K differently).  The
    sweep itself must not depend on the launch a leaf is in: wherever the two fits left the same factor bits, Z and mll are the
    same bits.  (A COPY leaf counts with its source's factor.)"""
    T = TABLE
    assert T["op"][CPY] == 1 and T["src"][CPY] == SRC and T["op"][PRE] == 2
    Y, mean = _table_targets()
    try:
        _table_setup(ctx, lanes=1, joint=True)
        one = _table_run(ctx, Y, mean)
        assert ctx.lanes() == 1
        ref = _table_reference(ctx, Y, mean)
        _table_check("table, one lane, rows through the fit", T, ref, *one, Y)
        # the COPY leaf shares its source's factor: column 0 (same targets, same mean) gives the same bits, the others do not
        assert _same_bits(one[2][CPY][:, 0], one[2][SRC][:, 0]) and not _same_bits(one[2][CPY][:, 1], one[2][SRC][:, 1])
        _table_setup(ctx, lanes=1, joint=False)
        alone = _table_run(ctx, Y, mean)
        F1 = _factors(ctx)
        _table_check("table, one lane, standalone sweep", T, ref, *alone, Y)
        _check("mu, route against route", alone[1], one[1], 2.0 * td.mu_tol(one[1], np.max(np.abs(Y), axis=0, keepdims=True)))
        _table_setup(ctx, lanes=2, joint=False)
        two = _table_run(ctx, Y, mean)
        assert ctx.lanes() == 2
        F2 = _factors(ctx)
        _table_check("table, two lanes, standalone sweep", T, ref, *two, Y)
        same = [l for l in range(T["kid"].size) if _same_bits(F1[l], F2[l])]
        print(f"\nleaves whose factors are the same bits under one and two lanes: {len(same)} of {T['kid'].size}")
        assert same, "no leaf keeps its factor bits across lane counts: nothing to compare the sweep on"
        for l in same:
            assert _same_bits(alone[2][l], two[2][l]) and _same_bits(alone[0][l], two[0][l]), l
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)
        ctx.set_joint(True)


# ------------------------------------------------------------------------------------- (4) consistency, bits

def test_consistency_with_the_primary_path(ctx):
    """Column j of Y = the y of set_train, mean = the leaf means: mll and mu agree with fit / predict_fetch at the dense
    tolerance (the orders of summation differ: no bit equality)."""
    T = TABLE
    Y, mean = _table_targets()
    Y = np.concatenate([Y[:, 1:2], Y[:, :1]], axis=1)       # the primary column second
    mean = np.concatenate([mean[:, 1:2], mean[:, :1]], axis=1)
    _table_setup(ctx)
    fmll, info, _ = ctx.fit()
    ctx.predict_run()
    pmu, _ = ctx.predict_fetch()
    mll, _ = ctx.solve_targets(Y, mean)
    mu = ctx.predict_targets()
    for l in range(T["kid"].size):
        n = int(T["obs_ptr"][l + 1] - T["obs_ptr"][l])
        F, _ = ctx.download_factor(l, n)
        cond = td.factor_cond(F)
        Z = ctx.targets_fetch(l)
        assert abs(mll[l, 1] - fmll[l]) <= 2.0 * td.mll_tol(Z, F, cond)[1], l
    _check("mu against predict_fetch", mu[:, 1], pmu, 2.0 * td.mu_tol(pmu[:, None], Y[:, 1:2])[:, 0])


def test_column_independence_and_repeatability(ctx):
    """Column j alone (Q = 1), inside Q = 5 and inside Q = 17 -- the other columns 1e6-scaled -- gives the same bits in Z, mll
    and mu; calling twice gives the same bits."""
    n, nt, D = 300, 130, 2
    rng = np.random.default_rng(11)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Xt = np.asfortranarray(rng.uniform(size=(nt, D)))
    col = _columns(3, X, 1)[:, 0]
    _single(ctx, X, col, 0.1, 0, np.array([np.log(0.4), 0.0]), np.log(0.1), Xt=Xt)
    ctx.predict_run()
    res = []
    for Q, j in ((1, 0), (5, 3), (17, 16)):
        Y = 1e6 * rng.standard_normal((n, Q))
        Y[:, j] = col
        mean = 1e6 * rng.standard_normal((1, Q))
        mean[0, j] = 0.1
        mll, _ = ctx.solve_targets(Y, mean)
        mu = ctx.predict_targets()
        Z = ctx.targets_fetch(0)
        mll2, _ = ctx.solve_targets(Y, mean)
        assert _same_bits(mll, mll2) and _same_bits(mu, ctx.predict_targets()) and _same_bits(Z, ctx.targets_fetch(0))
        res.append((Z[:, j].copy(), mll[0, j], mu[:, j].copy()))
    for r in res[1:]:
        assert _same_bits(r[0], res[0][0]) and _same_bits(r[1], res[0][1]) and _same_bits(r[2], res[0][2])


def test_nothing_else_moves(ctx):
    """fit outputs, predict_fetch, predict_cov, gradients, loo, loo_gradients and predict_gradients: the same bits before and
    after solve_targets / predict_targets."""
    T = TABLE
    Y, mean = _table_targets()
    stride = int(np.max(T["hyp_len"]))
    nt0 = int(T["route_ptr"][1] - T["route_ptr"][0])

    def everything():
        _table_setup(ctx)
        mll, info, _ = ctx.fit()
        ctx.predict_run()
        yield mll, info, *ctx.predict_fetch(), ctx.predict_cov(0, nt0)
        yield (ctx.gradients(stride), *ctx.loo(), *ctx.loo_gradients(stride), *ctx.predict_gradients(),
               *ctx.predict_fetch(), ctx.predict_cov(0, nt0), ctx.download_factor(CPY, int(T["obs_ptr"][CPY + 1] - T["obs_ptr"][CPY]))[1])

    base = [x for part in everything() for x in part]
    gen = everything()
    first = list(next(gen))
    ctx.solve_targets(Y, mean)
    ctx.predict_targets()
    got = first + list(next(gen))
    assert len(got) == len(base)
    for k, (p, q) in enumerate(zip(base, got)):
        assert _same_bits(p, q), k
    mll2, info2, _ = ctx.fit()
    assert _same_bits(mll2, base[0])


# ------------------------------------------------------------------------------------- (5) failures, states, arguments

def test_failed_leaf_gets_nan_and_the_others_are_unaffected(ctx):
    """Leaf 0: a rank-1 linear Gram of size 1e16 (not positive definite in float64, as tests/test_loo_gpu.py builds it); leaf 1:
    an ordinary IsoSE leaf."""
    n0, n1, nt = 140, 100, 7
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Xt = rng.uniform(size=(nt, 1))
    hyp1 = np.array([np.log(0.3), 0.0])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, np.concatenate([hyp1, [np.log(0.1)]]))
    ctx.set_test(Xt, [0, nt, 2 * nt], np.concatenate([np.arange(nt), np.arange(nt)]))
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    ctx.predict_run()
    Y = np.stack([y, np.cos(X[:, 0]) + 3.0], axis=1)
    mean = np.array([[0.0, 0.0], [0.2, 3.5]])
    mll, _ = ctx.solve_targets(Y, mean)
    mu = ctx.predict_targets()
    assert np.all(np.isnan(mll[0])) and np.all(np.isnan(mu[:nt]))
    rZ, rmll, rmu, cond, F = _dense_leaf(ctx, 1, 1, X[n0:], Y[n0:], mean[1], Xt)
    _check("good leaf Z", ctx.targets_fetch(1), rZ, 2.0 * td.z_tol(rZ, cond))
    _check("good leaf mll", mll[1], rmll, 2.0 * td.mll_tol(rZ, F, cond))
    _check("good leaf mu", mu[nt:], rmu, 2.0 * td.mu_tol(rmu, Y[n0:]))


def _code(fn):
    with pytest.raises(hipabi.DsmgpError) as e:
        fn()
    return e.value.code


def test_states_and_arguments():
    c = CASES["isose_n37"]
    X, Y, n = c["X"], c["Y"], c["X"].shape[0]
    ctx = hipabi.Context(0)
    try:
        ctx.set_train(X, Y[:, 0])
        ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
        ctx.set_hyper(0, 0, np.concatenate([c["loghyp"], [c["logNoise"]]]))
        assert _code(lambda: ctx.solve_targets(Y)) == hipabi.E_STATE                 # no fit
        ctx.fit()
        ctx.targets_Q = 3
        assert _code(ctx.predict_targets) == hipabi.E_STATE                         # no solve_targets
        assert _code(lambda: ctx.targets_fetch(0)) == hipabi.E_STATE
        assert _code(lambda: ctx.solve_targets(Y[:-1])) == hipabi.E_ARG              # N is not the N of set_train
        bad = Y.copy()
        bad[3, 1] = np.nan
        assert _code(lambda: ctx.solve_targets(bad)) == hipabi.E_ARG
        assert _code(lambda: ctx.solve_targets(Y, np.array([[0.0, np.inf, 0.0]]))) == hipabi.E_ARG
        import ctypes as C
        dp = hipabi._dp
        Yf = np.asfortranarray(Y)
        out = np.empty((1, 3), order="F")
        raw = lambda N, Q, ldy: ctx.lib.dsmgp_solve_targets(ctx.h, Yf.ctypes.data_as(dp), N, Q, ldy, None,       # noqa: E731
                                                            out.ctypes.data_as(dp), None)
        assert raw(n, 0, n) == hipabi.E_ARG and raw(n, 3, n - 1) == hipabi.E_ARG and raw(n + 1, 3, n + 1) == hipabi.E_ARG
        assert raw(n, 3, n) == 0                                                    # mean NULL = zeros, seconds NULL
        ref, _ = ctx.solve_targets(Y, np.zeros((1, 3)))
        assert _same_bits(out, ref)
        assert ctx.targets_fetch(0).shape == (n, 3)
        assert _code(lambda: ctx.targets_fetch(1)) == hipabi.E_ARG
        assert _code(ctx.predict_targets) == hipabi.E_STATE                         # no test set, no predict_run
        ctx.set_test(c["Xt"], [0, 0], np.zeros(0, dtype=np.int64))                  # no routed rows at all
        ctx.predict_run()
        assert ctx.predict_targets().shape == (0, 3)                                # success, nothing written
        nt = c["Xt"].shape[0]
        ctx.set_test(c["Xt"], [0, nt], np.arange(nt))
        assert _code(ctx.predict_targets) == hipabi.E_STATE                         # a new test set: predict_run first
        ctx.predict_run()
        mu = ctx.predict_targets()
        buf = np.empty((nt, 3), order="F")
        assert ctx.lib.dsmgp_predict_targets(ctx.h, buf.ctypes.data_as(dp), nt - 1, None) == hipabi.E_ARG
        sec = C.c_double(0.0)
        big = np.full((nt + 2, 3), -7.0, order="F")
        assert ctx.lib.dsmgp_predict_targets(ctx.h, big.ctypes.data_as(dp), nt + 2, C.byref(sec)) == 0
        assert _same_bits(big[:nt], mu) and np.all(big[nt:] == -7.0) and sec.value > 0.0
        ctx.fit()                                                                    # a later fit: Z is stale
        ctx.predict_run()
        assert _code(ctx.predict_targets) == hipabi.E_STATE and _code(lambda: ctx.targets_fetch(0)) == hipabi.E_STATE
        ctx.solve_targets(Y, np.zeros((1, 3)))
        assert _same_bits(ctx.predict_targets(), mu)                                # the context stays usable
        ctx.release()
        assert _code(lambda: ctx.solve_targets(Y)) == hipabi.E_STATE
        ctx.fit()
        ctx.solve_targets(Y[:, :1])                                                  # fewer columns: the arena is re-used
        assert ctx.targets_fetch(0).shape == (n, 1)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- (6) model API

def _model_case(family):
    X, y, Xt = dsm.regression_data(600, 2, n_test=24, seed=99)
    rng = np.random.default_rng(21)
    Y = np.stack([y, 5.0 + X[:, 0] - X[:, 1] ** 2, np.cos(4.0 * X[:, 1])], axis=1)
    Y[:, 1:] += 0.1 * rng.standard_normal((X.shape[0], 2))
    kern = dsm.IsoSE(np.log(0.4), 0.0)
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 2, 3, M=60, kernel=kern, logNoise=np.log(0.1), seed=3)
    elif family == "poe":
        m = dsm.buildPoE(X, y, 3, M=60, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), logNoise=np.log(0.1), seed=3)
    elif family == "rbcm":
        m = dsm.buildBCM(X, y, 3, M=60, kernel=kern, logNoise=np.log(0.1), robust=True, seed=3)
    else:
        X, Y = X[:200], Y[:200]
        m = dsm.GaussianProcess(X, Y[:, 0], kernel=kern, logNoise=np.log(0.1))
    return m, X, Y, Xt


@pytest.mark.parametrize("family", ["dsmgp", "poe", "rbcm", "gp"])
def test_model_api_against_refits(family):
    """predict_targets(model, xt)[...][:, j] against predict of the same model whose leaves were given y_j: a context refitted
    with y_j, the same tree, hypers and leaf means (not the code under test), aggregated by the model's own rule."""
    m, X, Y, Xt = _model_case(family)
    target = m.model if family == "gp" else m
    dsm.fit(m)
    if family == "dsmgp":
        dsm.update(m)
    table = dsm.fit_targets(m, Y)
    L, Q = target.L, Y.shape[1]
    assert table.shape == (L, Q)
    means = dsm.targets_leaf_means(m, Y)
    assert np.array_equal(means, np.stack([np.mean(Y[lf.obs], axis=0) for lf in target.leaves]))
    mu, var = dsm.predict_targets(m, Xt)
    assert mu.shape == (Xt.shape[0], Q) and var.shape == mu.shape
    rc = dmodel._routing(target, np.asfortranarray(Xt))
    ent = row_entries(rc["ptr"], rc["idx"], Xt.shape[0])
    fam, coef, group, G, plain, prior = dmodel._aggregation_spec(target)
    kw = dict(coef=coef, group=group, G=G, plain=plain)
    if fam == hipabi.AGG_RBCM:
        kw.update(kss_prior=dmodel._prior_diag(prior, Xt), noise_prior=float(np.exp(2 * prior.logNoise)))
    ref = hipabi.Context(0)
    try:
        ptr, idx = dmodel.obs_table(target.leaves)
        for j in range(Q):
            ref.set_train(X, Y[:, j])
            ref.set_leaves(ptr, idx, [lf.kernelid for lf in target.leaves], means[:, j])
            for lf in target.kernel_table():
                ref.set_hyper(lf.kernelid, lf.kernel.kind, np.concatenate([lf.kernel.loghyp(), [lf.logNoise]]))
            ref.set_test(Xt, rc["ptr"], rc["idx"])
            rmll, info, _ = ref.fit()
            assert np.all(info == 0)
            ref.predict_run()
            mu_l, var_l = ref.predict_fetch()
            am, av = ref.aggregate(fam, coef, group, G, plain=plain, prior_kernel_id=prior.kernelid if prior else 0)
            if family == "gp":
                am, av = mu_l, np.where(var_l <= 0, 1e-8, var_l)
            kss = np.full(mu_l.size, 1.0)
            tm, tv = moment_tol(mu_l, var_l, kss, 0.01, max(1.0, float(np.max(np.abs(Y[:, j])))))
            S1 = None
            if fam == hipabi.AGG_MIXTURE:
                S1 = np.array([sum(coef[l] * mu_l[e] ** 2 for l, e in er) for er in ent])
            if family == "gp":
                atm, atv = tm, tv
            else:
                atm, atv = agg_tol(fam, mu_l, var_l, tm, tv, ent, S1=S1, **kw)
            _check(f"{family} column {j} mu", mu[:, j], am, 2.0 * atm)
            _check(f"{family} column {j} var", var[:, j], av, 2.0 * atv)
            for l in range(L):
                F, _ = ref.download_factor(l, target.leaves[l].nobs)
                Zl = target.ctx.targets_fetch(l)
                assert abs(table[l, j] - rmll[l]) <= 2.0 * td.mll_tol(Zl, F, td.factor_cond(F))[j], (family, l, j)
    finally:
        ref.close()
