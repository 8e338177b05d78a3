"""GPU tests of dsmgp_mll_columns_gradients: hyper-parameter gradients of the weighted sum of the per-column log marginal
likelihoods of dsmgp_solve_targets, through hipabi.Context.targets_gradients.

References: tests/golden/gp_targets_grad.npz (50 digits, tests/golden/make_targets_grad_golden.py) for single leaves; the
float64 dense restatement tests/targets_grad_dense.py for the wide inputs; dsmgp_gradients after a refit per column (the
existing path, not the code under test) for the agreement checks.  Tolerance: targets_grad_dense.tolerance -- the project's
rule for a gradient component per column, carried through the weighted sum -- doubled where both sides are float64."""
import os

import numpy as np
import pytest

import targets_dense as td
import targets_grad_dense as tgd
from deepstructuredmixtures_amd import hipabi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = tgd.load_cases()
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check(tag, got, ref, tol):
    got, ref = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, ref))
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err = np.abs(got - ref)
    ratio = err / tol
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    assert np.all(err <= tol), (tag, got, ref, tol)
    return float(np.max(ratio))


def _single(ctx, X, y, mean, kind, hyp):
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(mean)])
    ctx.set_hyper(0, int(kind), hyp)
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    return mll


def _one_hot(Q, j):
    w = np.zeros(Q)
    w[j] = 1.0
    return w


# ------------------------------------------------------------------------------------- (1) the 50-digit fixture

@pytest.mark.parametrize("fused_gram", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_against_50_digit_references(ctx, name, fused_gram):
    """Every case of gp_targets_grad.npz: the signed weighted sum, unit weights (NULL) and one-hot weights of the first, the
    second and the last column, with the Gram values from the Gram launch and fused into the update; ArdSE with the true
    length-scale gradient off (exact zeros) and on."""
    c = CASES[name]
    kind, hyp, Y, w = int(c["kind"]), c["hyp"], c["Y"], c["w"]
    n, D = c["X"].shape
    Q = Y.shape[1]
    ctx.set_option(hipabi.OPT_FUSED_GRAM, fused_gram)
    worst = 0.0
    try:
        variants = [(0, c["grad"], c["wsum"])]
        if kind == 1:
            Gt = c["grad"].copy()
            Gt[:, :D] = c["grad_true"]
            variants.append((1, Gt, np.concatenate([c["wsum_true"], c["wsum"][D:]])))
        for ard, G, wsum in variants:
            ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, ard)
            try:
                _single(ctx, c["X"], Y[:, 0], c["mean"][0], kind, hyp)
                mll, _ = ctx.solve_targets(Y, c["mean"][None, :])
                tolk = dict(kind=kind, hyp=hyp, weak=bool(c["weak"]), n=n, c_trKinv=float(c["c_trKinv"]))
                got = ctx.targets_gradients(hyp.size, w[None, :])[0]
                if kind == 1 and not ard:
                    assert np.all(got[:D] == 0.0)
                worst = max(worst, _check(f"{name} ard={ard} signed", got, wsum, tgd.tolerance(G, w, c["cond"], **tolk)))
                ones = np.ones(Q)
                worst = max(worst, _check(f"{name} ard={ard} ones", ctx.targets_gradients(hyp.size)[0], tgd.weighted(G, ones),
                                          tgd.tolerance(G, ones, c["cond"], **tolk)))
                for j in sorted({0, min(1, Q - 1), Q - 1}):
                    e = _one_hot(Q, j)
                    worst = max(worst, _check(f"{name} ard={ard} column {j}", ctx.targets_gradients(hyp.size, e[None, :])[0], G[j],
                                              tgd.tolerance(G, e, c["cond"], **tolk)))
            finally:
                ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
    print(f"\n{name} fused_gram={fused_gram}: worst err/tol {worst:.3g}")


# ------------------------------------------------------------------------------------- (2) wide inputs

def _columns(seed, X, Q):
    rng = np.random.default_rng(seed)
    j = np.arange(Q)
    return (np.sin((1.0 + j)[None, :] * X[:, :1]) * (1.0 + 0.5 * j)[None, :] + 3.0 * (j % 3)[None, :]
            + 0.1 * rng.standard_normal((X.shape[0], Q)))


@pytest.mark.parametrize("kind,D", [(0, 36), (4, 40), (8, 40), (10, 40)])
def test_wide_inputs_against_the_dense_reference(ctx, kind, D):
    """D = 36, IsoSE: the epilogue that reads the coordinates from global memory; D = 40 for ArdSEProduct, ArdMatern52 and ArdRQ:
    the chunked staging (two chunks of <= 35 dimensions).  n = 130 (a diagonal tile, an off-diagonal tile, padding), Q = 3."""
    n, Q = 130, 3
    rng = np.random.default_rng(400 + kind)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Y = _columns(kind, X, Q)
    mean = np.mean(Y, axis=0)
    ll = np.log(np.sqrt(D) * np.linspace(0.3, 0.6, D))
    h = {0: [np.log(0.3 * np.sqrt(D)), 0.1], 4: list(ll) + [0.0], 8: list(ll) + [0.1], 10: list(ll) + [np.log(2.0), 0.0]}[kind]
    hyp = np.array(h + [np.log(0.2)])
    _single(ctx, X, Y[:, 0], mean[0], kind, hyp)
    ctx.solve_targets(Y, mean[None, :])
    G, _, cond = tgd.column_gradients(kind, hyp, X, Y, mean)
    w = tgd.signed_weights(Q) + np.array([0.0, 0.0, 0.25])
    _check(f"kind {kind} D {D} signed", ctx.targets_gradients(hyp.size, w[None, :])[0], tgd.weighted(G, w),
           2.0 * tgd.tolerance(G, w, cond))
    _check(f"kind {kind} D {D} ones", ctx.targets_gradients(hyp.size)[0], tgd.weighted(G, np.ones(Q)),
           2.0 * tgd.tolerance(G, np.ones(Q), cond))


# ------------------------------------------------------------------------------------- (3), (4) the existing path, columns

_H3 = {0: [np.log(0.4), 0.1], 3: list(np.log([0.8, 1.2, 1.6])) + [0.0], 8: list(np.log([0.5, 0.8, 0.6])) + [-0.1]}


@pytest.mark.parametrize("kind", [0, 3, 8])
def test_agreement_with_gradients_after_refits(ctx, kind):
    """Q = 1 with column j equals dsmgp_gradients after set_train(y_j) and a refit; Y = [y_1 y_2 y_3] with one-hot and with
    signed weights equals the same combination of the three refits' rows -- within the summed tolerances, both sides float64."""
    n, D, Q = 300, 3, 3
    rng = np.random.default_rng(31 + kind)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Y = _columns(50 + kind, X, Q)
    mean = np.mean(Y, axis=0)
    hyp = np.array(_H3[kind] + [np.log(0.2)])
    G = np.zeros((Q, hyp.size))
    for j in range(Q):
        _single(ctx, X, Y[:, j], mean[j], kind, hyp)
        G[j] = ctx.gradients(hyp.size)[0]
        F, _ = ctx.download_factor(0, n)
        ctx.solve_targets(Y[:, j], mean[None, j:j + 1])
        _check(f"kind {kind} Q = 1, column {j}", ctx.targets_gradients(hyp.size)[0], G[j],
               2.0 * tgd.tolerance(G[j:j + 1], np.ones(1), td.factor_cond(F)))
    cond = td.factor_cond(F)
    ctx.solve_targets(Y, mean[None, :])
    for w in [_one_hot(Q, j) for j in range(Q)] + [np.array([1.5, -2.0, 0.75]), np.array([-1.0, 0.0, 1.0])]:
        _check(f"kind {kind} weights {w}", ctx.targets_gradients(hyp.size, w[None, :])[0], tgd.weighted(G, w),
               2.0 * tgd.tolerance(G, w, cond))


def test_a_column_does_not_depend_on_its_neighbours(ctx):
    """One-hot weight j at Q = 17 -- the other columns 1e3-scaled -- against Q = 1 with that column."""
    n, D, kind = 130, 3, 8
    rng = np.random.default_rng(77)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    col = _columns(9, X, 1)[:, 0]
    hyp = np.array(_H3[kind] + [np.log(0.2)])
    _single(ctx, X, col, 0.1, kind, hyp)
    F, _ = ctx.download_factor(0, n)
    cond = td.factor_cond(F)
    ctx.solve_targets(col, np.array([[0.1]]))
    alone = ctx.targets_gradients(hyp.size)[0]
    for j in (0, 15, 16):
        Y = 1e3 * rng.standard_normal((n, 17))
        Y[:, j] = col
        mean = rng.standard_normal((1, 17))
        mean[0, j] = 0.1
        ctx.solve_targets(Y, mean)
        _check(f"column {j} of 17", ctx.targets_gradients(hyp.size, _one_hot(17, j)[None, :])[0], alone,
               2.0 * tgd.tolerance(alone[None, :], np.ones(1), cond))


# ------------------------------------------------------------------------------------- (5) bits

def _table_setup(ctx, lanes=0):
    T = TABLE
    ctx.set_option(hipabi.OPT_LANES, lanes)
    ctx.set_train(T["X"], T["y"])
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean"])
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])
    ctx.set_test(T["Xt"], T["route_ptr"], T["route_idx"])


def _table_targets(Q=3):
    T = TABLE
    Y = np.concatenate([T["y"][:, None], _columns(7, T["X"], Q - 1)], axis=1)
    L = T["kid"].size
    mean = np.stack([np.mean(Y[T["obs_idx"][int(T["obs_ptr"][l]):int(T["obs_ptr"][l + 1])]], axis=0) for l in range(L)])
    mean[:, 0] = T["mean"]
    W = np.random.default_rng(3).uniform(-1.0, 2.0, size=(L, Q))
    return Y, mean, W


def _factors(ctx):
    T = TABLE
    return [np.tril(ctx.download_factor(l, int(T["obs_ptr"][l + 1] - T["obs_ptr"][l]))[0]) for l in range(T["kid"].size)]


def test_same_bits_from_call_to_call_and_across_lane_counts(ctx):
    """The 41-leaf table of gp_pred.npz (a COPY and a PREFIX leaf): two calls give the same bits, with the L^-T arena filled by
    the call and read as it is; one lane against two on every leaf whose factor bits agree under both fits."""
    T = TABLE
    Y, mean, W = _table_targets()
    stride = int(np.max(T["hyp_len"]))
    res, fac = [], []
    try:
        for lanes in (1, 2):
            _table_setup(ctx, lanes=lanes)
            _, info, _ = ctx.fit()
            assert np.all(info == 0) and ctx.lanes() == lanes
            ctx.solve_targets(Y, mean)
            g = ctx.targets_gradients(stride, W)
            assert np.all(np.isfinite(g))
            assert _same_bits(g, ctx.targets_gradients(stride, W))
            ctx.gradients(stride)                       # the gradient pass inverts again: the arena is rewritten in between
            assert _same_bits(g, ctx.targets_gradients(stride, W))
            res.append(g)
            fac.append(_factors(ctx))
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)
    same = [l for l in range(T["kid"].size) if _same_bits(fac[0][l], fac[1][l])]
    print(f"\nleaves whose factors are the same bits under one and two lanes: {len(same)} of {T['kid'].size}")
    assert same, "no leaf keeps its factor bits across lane counts: nothing to compare on"
    for l in same:
        assert _same_bits(res[0][l], res[1][l]), l


# ------------------------------------------------------------------------------------- (6) every kind in one context

_HYP = [
    [np.log(0.4), 0.1, np.log(0.2)],                                     # 0 IsoSE
    list(np.log([0.4, 0.6, 0.9])) + [-0.3, np.log(0.2)],                 # 1 ArdSE
    [np.log(1.0), 0.0, np.log(0.2)],                                     # 2 IsoLinear
    list(np.log([0.8, 1.2, 1.6])) + [0.0, np.log(0.2)],                  # 3 ArdLinear
    list(np.log([0.5, 0.7, 0.9])) + [0.0, np.log(0.2)],                  # 4 ArdSEProduct
    [np.log(0.5), 0.0, np.log(0.2)],                                     # 5 IsoMatern32
    [np.log(0.7), 0.2, np.log(0.2)],                                     # 6 IsoMatern52
    list(np.log([0.5, 0.7, 0.9])) + [0.1, np.log(0.2)],                  # 7 ArdMatern32
    list(np.log([0.5, 0.8, 0.6])) + [-0.1, np.log(0.2)],                 # 8 ArdMatern52
    [np.log(0.5), np.log(2.0), 0.0, np.log(0.2)],                        # 9 IsoRQ
    list(np.log([0.5, 0.7, 0.9])) + [np.log(0.3), -0.1, np.log(0.2)],    # 10 ArdRQ
]


def test_every_kernel_kind_in_one_context_equals_each_leaf_alone(ctx):
    """Kernel ids 0..10 = the eleven kinds (ArdSE with the true length-scale gradient) in one leaf table, leaves of n = 2, 130
    and 300 for each, COPY leaves with their source's mean row and with a mean row of their own, and a PREFIX leaf (a second block of its own); weights per
    (leaf, column).  Every row equals the same leaf alone in a context to 1e-12 relative (task dealing reorders the sums)."""
    N, D, Q = 3000, 3, 5
    rng = np.random.default_rng(86)
    X = np.asfortranarray(rng.uniform(size=(N, D)))
    Y = _columns(86, X, Q)
    obs, kid = [], []
    for k in range(11):
        for n in (2, 130, 300):
            obs.append(np.sort(rng.choice(N, size=n, replace=False)))
            kid.append(k)
    L0 = len(obs)
    op, src, plen = [0] * L0, [-1] * L0, [0] * L0
    obs[13] = np.sort(rng.choice(2000, size=130, replace=False))       # the source of the PREFIX leaf below: rows below 2000
    means = [np.mean(Y[o], axis=0) for o in obs]
    # COPY leaves: IsoSE n = 300 and ArdLinear n = 130 with the source's mean row; ArdMatern52 n = 300 and ArdRQ n = 130 with their own
    for s, own in ((2, False), (10, False), (26, True), (31, True)):
        obs.append(obs[s].copy())
        kid.append(kid[s])
        means.append(means[s] + (0.3 * np.arange(1, Q + 1) if own else 0.0))
        op.append(1)
        src.append(s)
        plen.append(0)
    # a PREFIX leaf of the ArdSEProduct n = 130 leaf: the source's rows (all below row 2000), then 80 later rows of its own
    s = 13
    obs.append(np.concatenate([obs[s], 2000 + np.sort(rng.choice(N - 2000, size=80, replace=False))]))
    kid.append(kid[s])
    means.append(np.mean(Y[obs[-1]], axis=0))
    op.append(2)
    src.append(s)
    plen.append(obs[s].size)
    L = len(obs)
    W = rng.uniform(-1.0, 2.0, size=(L, Q))
    W[3, 2] = 0.0
    stride = D + 3

    def setup(c, leaves):
        c.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
        c.set_train(X, Y[:, 0])
        sel = [obs[i] for i in leaves]
        c.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in sel])]), np.concatenate(sel),
                     [kid[i] for i in leaves], [float(means[i][0]) for i in leaves])
        for k in range(11):
            c.set_hyper(k, k, _HYP[k])

    mixed = hipabi.Context(0)
    try:
        setup(mixed, range(L))
        mixed.set_sharing(op, src, np.array(plen, dtype=np.int64))
        _, info, _ = mixed.fit()
        assert np.all(info == 0)
        mixed.solve_targets(Y, np.stack(means))
        full = mixed.targets_gradients(stride, W)
    finally:
        mixed.close()
    try:
        alone = np.zeros((L, stride))
        for i in range(L):
            setup(ctx, [i])
            _, info, _ = ctx.fit()
            assert info[0] == 0
            ctx.solve_targets(Y, means[i][None, :])
            alone[i] = ctx.targets_gradients(stride, W[i:i + 1])[0]
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    scale = np.max(np.abs(alone), axis=1)
    assert np.all(scale > 0)
    rel = np.max(np.abs(full - alone), axis=1) / scale
    print(f"\n{L} leaves: worst relative difference {np.max(rel):.3g} (leaf {int(np.argmax(rel))})")
    assert np.all(rel <= 1e-12), (int(np.argmax(rel)), float(np.max(rel)))
    for i in range(L):
        assert np.all(full[i, len(_HYP[kid[i]]):] == 0.0)


# ------------------------------------------------------------------------------------- (7) non-interference

def test_nothing_else_moves(ctx):
    """gradients, loo_gradients, predict_fetch and targets_fetch, also under a set_gradient_leaves mask: the same bits before
    and after targets_gradients; so are fit's outputs, loo, predict_targets and predict_gradients."""
    T = TABLE
    L = T["kid"].size
    Y, mean, W = _table_targets()
    stride = int(np.max(T["hyp_len"]))
    mask = np.arange(L) % 3 != 1

    def everything(call):
        _table_setup(ctx)
        out = list(ctx.fit()[:2])
        ctx.predict_run()
        ctx.solve_targets(Y, mean)
        if call:
            ctx.targets_gradients(stride, W)
        out += [ctx.gradients(stride), *ctx.loo_gradients(stride), *ctx.predict_fetch(), *ctx.loo(), ctx.predict_targets(),
                *ctx.predict_gradients()]
        out += [ctx.targets_fetch(l) for l in (0, L - 1)]
        ctx.set_gradient_leaves(mask)
        try:
            if call:
                ctx.targets_gradients(stride, W)
            masked = ctx.gradients(stride)
            assert np.all(masked[~mask] == 0.0)
            if call:
                assert np.all(np.any(ctx.targets_gradients(stride, W)[~mask] != 0.0, axis=1))      # the mask does not apply
            out += [masked, ctx.gradients(stride), *ctx.loo_gradients(stride), *ctx.predict_fetch(), ctx.targets_fetch(0)]
        finally:
            ctx.set_gradient_leaves(None)
        return out

    base = everything(False)
    got = everything(True)
    assert len(base) == len(got)
    for k, (p, q) in enumerate(zip(base, got)):
        assert _same_bits(p, q), k


# ------------------------------------------------------------------------------------- (8) states, arguments, failures

def _code(fn):
    with pytest.raises(hipabi.DsmgpError) as e:
        fn()
    return e.value.code


def test_states_and_arguments():
    c = CASES["isose_n128_q16"]
    X, Y, n, hyp = c["X"], c["Y"][:, :3], c["X"].shape[0], c["hyp"]
    ctx = hipabi.Context(0)
    try:
        ctx.set_train(X, Y[:, 0])
        ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
        ctx.set_hyper(0, 0, hyp)
        ctx.targets_Q = 3
        assert _code(lambda: ctx.targets_gradients(3)) == hipabi.E_STATE            # no fit
        ctx.fit()
        assert _code(lambda: ctx.targets_gradients(3)) == hipabi.E_STATE            # no solve_targets
        ctx.solve_targets(Y, np.zeros((1, 3)))
        ref = ctx.targets_gradients(3)
        assert _code(lambda: ctx.targets_gradients(2)) == hipabi.E_ARG              # stride smaller than the hyper-vector
        for bad in (np.nan, np.inf):
            assert _code(lambda: ctx.targets_gradients(3, np.array([[1.0, bad, 1.0]]))) == hipabi.E_ARG
        g = np.zeros((1, 3))
        assert ctx.lib.dsmgp_mll_columns_gradients(ctx.h, None, 3, None, None) == hipabi.E_ARG
        assert ctx.lib.dsmgp_mll_columns_gradients(ctx.h, g.ctypes.data_as(hipabi._dp), 3, None, None) == 0     # seconds NULL
        assert _same_bits(g, ref) and ctx.targets_gradients_seconds > 0.0
        assert _same_bits(ctx.targets_gradients(5)[:, :3], ref) and np.all(ctx.targets_gradients(5)[:, 3:] == 0.0)
        ctx.fit()                                                                    # a later fit: Z is stale
        assert _code(lambda: ctx.targets_gradients(3)) == hipabi.E_STATE
        ctx.solve_targets(Y, np.zeros((1, 3)))
        assert _same_bits(ctx.targets_gradients(3), ref)                            # the context stays usable
        ctx.release()
        assert _code(lambda: ctx.targets_gradients(3)) == hipabi.E_STATE
        ctx.fit()
        ctx.solve_targets(Y[:, :1], np.zeros((1, 1)))
        assert ctx.targets_gradients(3).shape == (1, 3)
    finally:
        ctx.close()


def test_under_a_reserved_pool_the_same_bits(ctx):
    """With dsmgp_reserve the A arena comes from the pool's stack: the same bits as without a pool, also after a new test set
    has reset the stack above the plan (the arenas of the targets go with it) and after dsmgp_release."""
    c = CASES["isose_n300_q33"]
    X, Y, hyp, w, n = c["X"], c["Y"], c["hyp"], c["w"], c["X"].shape[0]
    _single(ctx, X, Y[:, 0], c["mean"][0], 0, hyp)
    ctx.solve_targets(Y, c["mean"][None, :])
    ref = ctx.targets_gradients(hyp.size, w[None, :])
    pooled = hipabi.Context(0)
    try:
        pooled.reserve(1 << 28)
        _single(pooled, X, Y[:, 0], c["mean"][0], 0, hyp)
        assert _code(lambda: pooled.targets_gradients(hyp.size)) == hipabi.E_STATE
        pooled.solve_targets(Y, c["mean"][None, :])
        assert _same_bits(pooled.targets_gradients(hyp.size, w[None, :]), ref)
        pooled.set_test(X[:5], [0, 5], np.arange(5))            # the stack above the plan is reset
        assert _code(lambda: pooled.targets_gradients(hyp.size)) == hipabi.E_STATE
        pooled.fit()
        pooled.solve_targets(Y, c["mean"][None, :])
        assert _same_bits(pooled.targets_gradients(hyp.size, w[None, :]), ref)
        assert _same_bits(pooled.gradients(hyp.size), ctx.gradients(hyp.size))
        pooled.release()
        pooled.fit()
        pooled.solve_targets(Y[:, :3], c["mean"][None, :3])
        ctx.solve_targets(Y[:, :3], c["mean"][None, :3])
        assert _same_bits(pooled.targets_gradients(hyp.size), ctx.targets_gradients(hyp.size))
    finally:
        pooled.close()


def test_ardse_option_refusal_above_the_staging_limit():
    """ArdSE, DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT on, D = 36: DSMGP_E_ARG as dsmgp_gradients gives it; off: the call goes through."""
    n, D = 40, 36
    rng = np.random.default_rng(8)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Y = _columns(8, X, 2)
    hyp = np.array(list(np.log(np.sqrt(D) * np.linspace(0.3, 0.6, D))) + [0.0, np.log(0.2)])
    ctx = hipabi.Context(0)
    try:
        _single(ctx, X, Y[:, 0], 0.0, 1, hyp)
        ctx.solve_targets(Y, np.zeros((1, 2)))
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
        assert _code(lambda: ctx.gradients(hyp.size)) == hipabi.E_ARG
        assert _code(lambda: ctx.targets_gradients(hyp.size)) == hipabi.E_ARG
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
        g = ctx.targets_gradients(hyp.size)[0]
        assert np.all(g[:D] == 0.0) and np.all(np.isfinite(g)) and g[D + 1] != 0.0
    finally:
        ctx.close()


def test_failed_leaf_gets_a_nan_row_and_the_others_are_unaffected(ctx):
    """Leaf 0: a rank-1 linear Gram of size 1e16 (not positive definite in float64, as tests/test_targets_gpu.py builds it);
    leaf 1: an ordinary IsoSE leaf, which equals itself alone in a context."""
    n0, n1 = 140, 100
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Y = np.stack([y, np.cos(X[:, 0]) + 3.0], axis=1)
    mean = np.array([[0.0, 0.0], [0.2, 3.5]])
    W = np.array([[1.0, 1.0], [0.5, -2.0]])
    hyp1 = np.array([np.log(0.3), 0.0, np.log(0.1)])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, hyp1)
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    ctx.solve_targets(Y, mean)
    g = ctx.targets_gradients(3, W)
    assert np.all(np.isnan(g[0])) and np.all(np.isfinite(g[1]))
    G, _, cond = tgd.column_gradients(0, hyp1, X[n0:], Y[n0:], mean[1])
    _check("good leaf", g[1], tgd.weighted(G, W[1]), 2.0 * tgd.tolerance(G, W[1], cond))
    _, info, _ = ctx.fit()                                                          # the context stays usable
    ctx.solve_targets(Y, mean)
    assert _same_bits(ctx.targets_gradients(3, W)[1], g[1])
