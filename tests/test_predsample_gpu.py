"""GPU tests of dsmgp_predict_sample / dsmgp_predict_cov_factor (csrc/kernels_sample.hpp): joint draws of every leaf GP over its
routed rows, out = mu + chol(Sigma_l + jitter I) eps_l.  The bounds are derived in tests/predsample_dense.py; nothing here compares
against a tolerance read off the device."""
import ctypes as C
import math

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi, datagen, model as dmodel
from predsample_dense import check_draws, check_factor, same_bits, sun_column_bounds

pytestmark = pytest.mark.gpu

N, D = 200, 2           # two block rows of training data, the second partial
X = datagen.uniform(101, 0, N * D).reshape((N, D), order="F")
Y = np.sin(5 * X[:, 0]) + 0.5 * X[:, 1] + 0.1 * datagen.normal(102, 0, N)
XT = datagen.uniform(103, 0, 300 * D).reshape((300, D), order="F")
MEAN = float(np.mean(Y))
KINDS = {"isose": (0, [math.log(0.5), 0.0]), "isolinear": (2, [0.0, 0.0])}
NTS = (1, 16, 127, 128, 129, 257, 300)      # 1, 2 and 3 block steps, full and partial last block
COLS = (1, 15, 16, 17, 40)                  # the 16-column tile: partial, full, one over, several groups
JITTER = 1e-8


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _eps(seed, n, S):
    return datagen.normal(seed, 0, n * S).reshape((n, S), order="F")


def _single(ctx, kind, logNoise, nt, path):
    """Fit + predict the one leaf on the first nt test rows by either route to K_tn L^-T; returns mu."""
    k, h = KINDS[kind]
    ctx.set_train(X, Y)
    ctx.set_leaves([0, N], np.arange(N), [0], [MEAN])
    ctx.set_sharing(None, None, None)
    ctx.set_hyper(0, k, h + [float(logNoise)])
    Xt = np.asfortranarray(XT[:nt])
    if path == "joint":
        ctx.set_test(Xt, [0, nt], np.arange(nt))
        _, info, _ = ctx.fit()
        ctx.predict_run()
    else:
        _, info, _ = ctx.fit()
        ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
    assert info[0] == 0
    return ctx.predict_fetch()[0]


def _A(ctx, leaf, nt, with_noise, jitter):
    A = ctx.predict_cov(leaf, nt, with_noise)
    A[np.arange(nt), np.arange(nt)] += jitter
    return A


# ------------------------------------------------------------------------------------- single leaf

@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("logNoise", [-1.0, -3.0])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_factor_and_draws_by_test_set_size(ctx, kind, logNoise, path):
    """Checks 1 and 2 for every test-set size, with and without noise: the factor against A = predict_cov + jitter I formed on the
    host, the draws against mu + C eps from the device's own factor."""
    for nt in NTS:
        mu = _single(ctx, kind, logNoise, nt, path)
        for with_noise in (False, True):
            jitter = 0.0 if with_noise else JITTER
            eps = _eps(7 + nt, nt, 17)
            out, info = ctx.predict_sample(eps, with_noise=with_noise)
            assert info.shape == (1,) and info[0] == 0 and out.shape == (nt, 17) and out.flags.f_contiguous
            Cf = ctx.predict_cov_factor(0, nt)
            tag = f"{kind} logNoise={logNoise} {path} nt={nt} noise={with_noise}"
            check_factor(tag, _A(ctx, 0, nt, with_noise, jitter), Cf)
            check_draws(tag, out, mu, Cf, eps)


@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_draw_columns(ctx, kind, path):
    """Every column count around the 16-column tile, check 2, and the columns of the widest call are the bits of the others."""
    nt = 129
    mu = _single(ctx, kind, -1.0, nt, path)
    eps = _eps(5, nt, max(COLS))
    wide, _ = ctx.predict_sample(eps, with_noise=True)
    Cf = ctx.predict_cov_factor(0, nt)
    for S in COLS:
        out, info = ctx.predict_sample(eps[:, :S], with_noise=True)
        assert info[0] == 0 and out.shape == (nt, S)
        check_draws(f"{kind} {path} S={S}", out, mu, Cf, eps[:, :S])
        assert same_bits(out, wide[:, :S])
    one, _ = ctx.predict_sample(eps[:, 3], with_noise=True)         # a vector is one draw
    assert same_bits(one[:, 0], wide[:, 3])


@pytest.mark.parametrize("path", ["standalone", "joint"])
def test_bits(ctx, path):
    nt, S = 257, 40
    _single(ctx, "isose", -1.0, nt, path)
    before = (ctx.predict_fetch(), ctx.predict_cov(0, nt, True), ctx.predict_cov(0, nt, False), ctx.predict_gradients())
    eps = _eps(11, nt, S)
    a, _ = ctx.predict_sample(eps, with_noise=False)
    Ca = ctx.predict_cov_factor(0, nt)
    b, _ = ctx.predict_sample(eps, with_noise=False)                # the cached factor
    assert same_bits(a, b)
    n, _ = ctx.predict_sample(eps, with_noise=True)                 # another tag: factorised again ...
    assert not same_bits(a, n) and not same_bits(Ca, ctx.predict_cov_factor(0, nt))
    c, _ = ctx.predict_sample(eps, with_noise=False)                # ... and back
    assert same_bits(a, c) and same_bits(Ca, ctx.predict_cov_factor(0, nt))
    j, _ = ctx.predict_sample(eps, with_noise=False, jitter=1e-6)   # the jitter is part of the tag
    assert not same_bits(a, j)
    c, _ = ctx.predict_sample(eps, with_noise=False)
    assert same_bits(a, c)
    for s in (0, 15, 16, 39):
        one, _ = ctx.predict_sample(eps[:, s:s + 1], with_noise=False)
        assert same_bits(one[:, 0], a[:, s])
        other = _eps(12, nt, S)
        other[:, s] = eps[:, s]
        o, _ = ctx.predict_sample(other, with_noise=False)
        assert same_bits(o[:, s], a[:, s]) and not same_bits(o, a)
    after = (ctx.predict_fetch(), ctx.predict_cov(0, nt, True), ctx.predict_cov(0, nt, False), ctx.predict_gradients())
    for x, y in zip(before, after):
        if isinstance(x, tuple):
            assert all(same_bits(p, q) for p, q in zip(x, y))
        else:
            assert same_bits(x, y)


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("logNoise", [-1.0, -3.0])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_draws_against_lapack(ctx, kind, logNoise, with_noise):
    """Check 3: posterior_sample(device=True) against posterior_sample(device=False) (Sigma downloaded, LAPACK, the product on the
    host) at n_t = 300, column by column within Sun's perturbation bound for the two Cholesky factors plus the bound of check 2;
    the condition numbers the bound needs are asserted, not assumed."""
    nt, ns = 300, 5
    kern = dsm.IsoSE(math.log(0.5), 0.0) if kind == "isose" else dsm.IsoLinear(0.0)
    gp = dsm.GaussianProcess(X, Y, mean=dsm.ConstMean(MEAN), kernel=kern, logNoise=logNoise, run_cholesky=True, ctx=ctx)
    host = dsm.posterior_sample(gp, XT, ns, seed=3, with_noise=with_noise)
    dev = dsm.posterior_sample(gp, XT, ns, seed=3, with_noise=with_noise, device=True)
    assert dev.shape == (ns, nt) and same_bits(dev, dsm.posterior_sample(gp, XT, ns, seed=3, with_noise=with_noise, device=True))
    Cd = ctx.predict_cov_factor(0, nt)
    A = _A(ctx, 0, nt, with_noise, 0.0 if with_noise else dmodel.EPS)
    mu = ctx.predict_fetch()[0]
    eps = _eps(3, nt, ns)
    bounds, kappa, e_dev, e_host = sun_column_bounds(A, Cd, np.linalg.cholesky(A), eps, mu)
    diff = np.linalg.norm(dev.T - host.T, axis=0)
    print(f"\n{kind} logNoise={logNoise} noise={with_noise}: kappa_2(A) = {kappa:.3g}, eps_dev = {e_dev:.3g}, eps_host = {e_host:.3g}, "
          f"max ||delta||_2 = {np.max(diff):.3g}, worst / bound = {np.max(diff / bounds):.3g}")
    assert kappa <= (100.0 if with_noise else 1e8)
    assert np.all(diff <= bounds)


# ------------------------------------------------------------------------------------- a leaf table in one call

def _table():
    """Six leaves over 540 training rows: FULL (260 routed rows), its COPY (129), its PREFIX continuation (128), a FULL leaf with one
    routed row, a FULL leaf without routed rows, and a leaf whose fit fails (the rank-1 linear Gram of size 1e16 of
    test_not_positive_definite_is_reported) with 129 routed rows: block steps 0, 1 and 2 of the factorisation see four, two and one
    healthy leaves."""
    Xh = datagen.uniform(201, 0, 400 * D).reshape((400, D), order="F")
    Xf = np.zeros((140, D))
    Xf[:, 0] = np.linspace(1.0, 2.0, 140) * 1e8
    Xa = np.asfortranarray(np.vstack([Xh, Xf]))
    ya = np.concatenate([np.sin(4 * Xh[:, 0]) + Xh[:, 1] + 0.1 * datagen.normal(202, 0, 400), np.zeros(140)])
    obs = [np.arange(200), np.arange(200), np.arange(260), np.arange(260, 400), np.arange(100, 300), np.arange(400, 540)]
    op, src, plen = [0, 1, 2, 0, 0, 0], [-1, 0, 0, -1, -1, -1], [0, 0, 200, 0, 0, 0]
    kid = [0, 0, 0, 0, 0, 1]
    m0 = float(np.mean(ya[:200]))
    mean = [m0, m0, float(np.mean(ya[:260])), float(np.mean(ya[260:400])), 0.0, 0.0]
    routes = [np.arange(260), np.arange(100, 229), np.arange(128), np.array([7]), np.zeros(0, dtype=np.int64), np.arange(129)]
    return Xa, ya, obs, op, src, plen, kid, mean, routes


def _run_table(ctx, path, routes, eps_leaf, with_noise):
    Xa, ya, obs, op, src, plen, kid, mean, _ = _table()
    ctx.set_train(Xa, ya)
    ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), kid, mean)
    ctx.set_sharing(op, src, plen)
    ctx.set_hyper(0, 0, [math.log(0.5), 0.0, -1.0])
    ctx.set_hyper(1, 2, [0.0, 0.0, -30.0])
    rp = np.concatenate([[0], np.cumsum([r.size for r in routes])])
    ri = np.concatenate(routes).astype(np.int64)
    if path == "joint":
        ctx.set_test(XT, rp, ri)
        _, finfo, _ = ctx.fit()
        ctx.predict_run()
    else:
        _, finfo, _ = ctx.fit()
        ctx.predict_leaves(XT, rp, ri)
    assert np.all(finfo[:5] == 0) and finfo[5] > 0
    eps = np.asfortranarray(np.vstack([eps_leaf[l][:routes[l].size] for l in range(6)]))
    out, info = ctx.predict_sample(eps, with_noise=with_noise)
    return rp, eps, out, info


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("path", ["joint", "standalone"])
def test_leaf_table_in_one_call(ctx, path, lanes):
    S = 17
    routes = _table()[8]
    eps_leaf = [_eps(300 + l, 260, S) for l in range(6)]
    ctx.set_option(hipabi.OPT_LANES, lanes)
    try:
        for with_noise in (False, True):
            rp, eps, out, info = _run_table(ctx, path, routes, eps_leaf, with_noise)
            assert ctx.lanes() == lanes
            assert list(info) == [0, 0, 0, 0, 0, -1]
            mu = ctx.predict_fetch()[0]
            jitter = 0.0 if with_noise else JITTER
            for l in range(4):
                a, b = int(rp[l]), int(rp[l + 1])
                Cf = ctx.predict_cov_factor(l, b - a)
                tag = f"table {path} lanes={lanes} noise={with_noise} leaf {l}"
                check_factor(tag, _A(ctx, l, b - a, with_noise, jitter), Cf)
                check_draws(tag, out[a:b], mu[a:b], Cf, eps[a:b])
            assert ctx.predict_cov_factor(4, 0).shape == (0, 0)
            assert np.all(np.isnan(out[rp[5]:rp[6]])) and np.all(np.isfinite(out[:rp[5]]))
            # the other leaves' bits do not depend on the failed leaf being in the call (a task belongs to one leaf and one
            # block step, whatever else the launch carries: equal bits, not rounding)
            without = routes[:5] + [np.zeros(0, dtype=np.int64)]
            rp2, _, out2, info2 = _run_table(ctx, path, without, eps_leaf, with_noise)
            assert list(info2) == [0, 0, 0, 0, 0, 0] and rp2[5] == rp[5]
            assert same_bits(out2, out[:rp[5]])
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)


# ------------------------------------------------------------------------------------- not positive definite, exact

@pytest.mark.parametrize("case", ["row131", "row2"])
def test_first_bad_minor_of_the_test_covariance_is_reported_exactly(ctx, case):
    """IsoLinear, l = 1, D = 132, logNoise = -1; training rows 2^27 e_131 and 2^27 e_130, so K_y = 2^54 I exactly (noise and jitter
    are absorbed: ulp(2^54) = 4); test rows 2^27 e_i: Sigma is 2^54 x their 0/1 Gram, every operation of the factorisation is exact
    and the pivot of the repeated row is exactly 0.  info must equal LAPACK's 131 (the second block step) resp. 2; a healthy leaf in
    the same call keeps its bits."""
    Dx = 132
    two27 = 2.0 ** 27
    Xs = np.zeros((2, Dx))
    Xs[0, 131] = Xs[1, 130] = two27
    Xh = datagen.uniform(401, 0, 50 * Dx).reshape((50, Dx), order="F")
    Xa = np.asfortranarray(np.vstack([Xs, Xh]))
    ya = np.concatenate([np.zeros(2), datagen.normal(402, 0, 50)])
    if case == "row131":
        T = np.zeros((131, Dx))
        T[np.arange(130), np.arange(130)] = two27
        T[130] = T[5]
        want = 131
    else:
        T = np.zeros((2, Dx))
        T[:, 0] = two27
        want = 2
    ns = T.shape[0]
    Th = datagen.uniform(403, 0, 40 * Dx).reshape((40, Dx), order="F")
    Xt = np.asfortranarray(np.vstack([T, Th]))
    G = (T @ T.T) / two27 ** 2
    import scipy.linalg as sla
    assert sla.lapack.dpotrf(2.0 ** 54 * G + 1e-8 * np.eye(ns), lower=1)[1] == want
    eps_s, eps_h = _eps(21, ns, 3), _eps(22, 40, 3)

    def run(with_singular):
        ctx.set_train(Xa, ya)
        ctx.set_leaves([0, 2, 52], np.arange(52), [0, 1], [0.0, 0.0])
        ctx.set_sharing(None, None, None)
        ctx.set_hyper(0, 2, [0.0, 0.0, -1.0])
        ctx.set_hyper(1, 0, [math.log(4.0), 0.0, -1.0])
        _, finfo, _ = ctx.fit()
        assert not np.any(finfo)
        k = ns if with_singular else 0
        ctx.predict_leaves(Xt, [0, k, k + 40], np.concatenate([np.arange(k), ns + np.arange(40)]))
        return k

    healthy = {}
    for with_noise in (False, True):
        run(False)
        healthy[with_noise], info = ctx.predict_sample(eps_h, with_noise=with_noise)
        assert not np.any(info)
    k = run(True)
    assert np.array_equal(ctx.predict_cov(0, ns, False), 2.0 ** 54 * G) and np.array_equal(ctx.predict_cov(0, ns, True), 2.0 ** 54 * G)
    for with_noise in (False, True):
        out, info = ctx.predict_sample(np.asfortranarray(np.vstack([eps_s, eps_h])), with_noise=with_noise)
        assert list(info) == [want, 0], (case, with_noise, list(info))
        assert np.all(np.isnan(out[:k]))
        assert same_bits(out[k:], healthy[with_noise])


# ------------------------------------------------------------------------------------- state and arguments

def _raw_sample(ctx, eps, ld_eps, S, out, ld_out, with_noise=0, jitter=0.0):
    dp = C.POINTER(C.c_double)
    return ctx.lib.dsmgp_predict_sample(ctx.h, with_noise, jitter, None if eps is None else eps.ctypes.data_as(dp), ld_eps, S,
                                        None if out is None else out.ctypes.data_as(dp), ld_out, None, None)


def test_state_and_arguments(ctx):
    nt = 129
    k, h = KINDS["isose"]
    ctx.set_train(X, Y)
    ctx.set_leaves([0, N], np.arange(N), [0], [MEAN])
    ctx.set_sharing(None, None, None)
    ctx.set_hyper(0, k, h + [-1.0])
    ctx.fit()
    Xt = np.asfortranarray(XT[:nt])
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    eps = _eps(1, nt, 3)
    with pytest.raises(hipabi.DsmgpError) as e:         # before predict_run
        ctx.predict_sample(eps)
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    with pytest.raises(hipabi.DsmgpError) as e:         # no factor yet
        ctx.predict_cov_factor(0, nt)
    assert e.value.code == hipabi.E_STATE
    good, info = ctx.predict_sample(eps)
    assert info[0] == 0
    out = np.empty((nt, 3), order="F")
    bad = eps.copy(order="F")
    bad[5, 1] = np.inf
    nan = eps.copy(order="F")
    nan[0, 2] = np.nan
    for args in ((eps, nt, 0, out, nt), (eps, nt, 65536, out, nt), (None, nt, 3, out, nt), (eps, nt, 3, None, nt),
                 (eps, nt - 1, 3, out, nt), (eps, nt, 3, out, nt - 1), (bad, nt, 3, out, nt), (nan, nt, 3, out, nt)):
        assert _raw_sample(ctx, *args) == hipabi.E_ARG, args[1:3]
    for jitter in (-1e-9, math.inf, math.nan):
        assert _raw_sample(ctx, eps, nt, 3, out, nt, jitter=jitter) == hipabi.E_ARG
    for leaf, m in ((1, nt), (-1, nt), (0, nt - 1)):
        with pytest.raises(hipabi.DsmgpError) as e:
            ctx.predict_cov_factor(leaf, m)
        assert e.value.code == hipabi.E_ARG
    assert same_bits(good, ctx.predict_sample(eps)[0])  # the refusals left the context as it was
    assert _raw_sample(ctx, eps, nt, 3, out, nt, jitter=JITTER) == 0 and same_bits(out, good)
    ctx.set_hyper(0, k, [h[0] + 0.1, h[1], -1.0])
    ctx.fit()                                           # a later fit: the rows rode along, predict_run has not finished them
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.predict_sample(eps)
    assert e.value.code == hipabi.E_STATE
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.predict_cov_factor(0, nt)
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    assert not same_bits(good, ctx.predict_sample(eps)[0])
    # no routed rows at all: success, nothing written
    ctx.set_test(Xt, [0, 0], np.zeros(0, dtype=np.int64))
    ctx.predict_run()
    empty, info = ctx.predict_sample(np.zeros((0, 4), order="F"))
    assert empty.shape == (0, 4) and info[0] == 0


def test_draws_on_the_grown_model(ctx):
    """After append_rows(keep_test=True) and the resumed predict_run the call works on the grown model: check 2 and check 1."""
    nt = 257
    mu0 = _single(ctx, "isose", -1.0, nt, "joint")
    eps = _eps(31, nt, 5)
    old, _ = ctx.predict_sample(eps, with_noise=True)
    Xn = datagen.uniform(104, 0, 70 * D).reshape((70, D), order="F")
    yn = np.sin(5 * Xn[:, 0]) + 0.5 * Xn[:, 1]
    _, info, _ = ctx.append_rows(Xn, yn, [0, 70], np.arange(70), keep_test=True)
    assert info[0] == 0
    with pytest.raises(hipabi.DsmgpError) as e:         # the factors fell with the prediction
        ctx.predict_sample(eps, with_noise=True)
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    mu = ctx.predict_fetch()[0]
    out, info = ctx.predict_sample(eps, with_noise=True)
    assert info[0] == 0 and not same_bits(out, old) and not same_bits(mu, mu0)
    Cf = ctx.predict_cov_factor(0, nt)
    check_factor("grown model", _A(ctx, 0, nt, True, 0.0), Cf)
    check_draws("grown model", out, mu, Cf, eps)


# ------------------------------------------------------------------------------------- the model API on the device

def test_mixture_sample_on_the_device():
    Xm, ym, Xq = dsm.regression_data(1500, 3, n_test=64, seed=4242)
    m = dsm.buildDSMGP(Xm, ym, 2, 4, M=40, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=1)
    ns = 4
    ptr, idx, draws, info = dsm.leaf_samples(m, Xq, ns, seed=8)
    assert not np.any(info) and draws.shape == (int(ptr[-1]), ns) and np.all(np.isfinite(draws))
    want = datagen.normal(8, 0, draws.size).reshape(draws.shape, order="F")
    mu, _ = m.ctx.predict_fetch()
    for l in range(m.L):
        a, b = int(ptr[l]), int(ptr[l + 1])
        if a < b:
            check_draws(f"model leaf {l}", draws[a:b], mu[a:b], m.ctx.predict_cov_factor(l, b - a), want[a:b])
    out = dsm.mixture_sample(m, Xq, ns, seed=8)
    assert out.shape == (ns, 64)
    leaf_of_entry = np.repeat(np.arange(m.L), np.diff(ptr))
    nodes, choices = dmodel._mixture_choices(m.root, ns, 8)
    for s in range(ns):
        chosen = dmodel._mixture_leaf_of_rows(m.root, Xq, nodes, choices[s])
        sets = {}
        for r in range(64):
            ents = np.nonzero(idx == r)[0]
            hits = [e for e in ents if draws[e, s] == out[s, r]]
            assert len(hits) == 1 and leaf_of_entry[hits[0]] == chosen[r]       # exactly one of the leaves the row is routed to
            key = tuple(leaf_of_entry[ents])
            assert sets.setdefault(key, chosen[r]) == chosen[r]                 # the choice depends on the sum nodes only
    saved = [nd.logweights.copy() for nd in nodes]
    try:
        for nd in nodes:                                # one-hot weights: leaf_samples at the selected leaves
            lw = np.full(len(nd.children), -np.inf)
            lw[0] = 0.0
            nd.logweights = lw
        nodes1, ch1 = dmodel._mixture_choices(m.root, ns, 8)
        assert not np.any(ch1)
        out1 = dsm.mixture_sample(m, Xq, ns, seed=8)
        chosen = dmodel._mixture_leaf_of_rows(m.root, Xq, nodes1, ch1[0])
        for r in range(64):
            seg = idx[ptr[chosen[r]]:ptr[chosen[r] + 1]]
            e = int(ptr[chosen[r]] + np.searchsorted(seg, r))
            assert idx[e] == r and same_bits(out1[:, r], draws[e, :])
    finally:
        for nd, lw in zip(nodes, saved):
            nd.logweights = lw
    m.ctx.close()
