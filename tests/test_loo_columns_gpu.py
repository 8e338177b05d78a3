"""GPU tests of dsmgp_loo_columns and dsmgp_loo_columns_gradients: leave-one-out moments and hyper-parameter gradients of the
target columns of dsmgp_solve_targets on one factorisation, through hipabi.Context.loo_targets / loo_targets_gradients and the
model functions on top of them.

References: tests/golden/gp_loo_columns.npz (50 digits, tests/golden/make_loo_columns_golden.py) for single leaves; the float64
dense restatement tests/loo_columns_dense.py for the sizes at which tiling can go wrong and for wide inputs; dsmgp_loo and
dsmgp_loo_gradients (the existing path, not the code under test) for the agreement checks.  Tolerances: loo_dense.loo_tol per
column for the moments, loo_grad_dense.tolerance per column carried through the weighted sum for the gradients
(loo_columns_dense.moment_tolerances / gradient_tolerance), doubled where both sides are float64."""
import os

import numpy as np
import pytest

import dense_kernels as dk
import loo_columns_dense as lcd
from deepstructuredmixtures_amd import hipabi

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = lcd.load_cases()
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


def _check_moments(tag, case, got, factor=1.0):
    mu, var, lpd = got
    worst = 0.0
    for q in range(case["Y"].shape[1]):
        tm, tv, _, ts = lcd.moment_tolerances(case, q)
        worst = max(worst, _check(f"{tag} mu column {q}", mu[:, q], case["mu"][:, q], factor * tm),
                    _check(f"{tag} lpd column {q}", lpd[0, q], case["lpd"][q], factor * ts))
    return max(worst, _check(f"{tag} var", var, case["var"], factor * tv))


# ------------------------------------------------------------------------------------- (1) the 50-digit fixture

@pytest.mark.parametrize("fused_gram", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_against_50_digit_references(ctx, name, fused_gram):
    """Every case of gp_loo_columns.npz through both calls: the moments and the lpd table; the fixture's weighted gradient (a
    zero weight where Q = 3), unit weights (NULL) and one-hot weights of the first and the last column."""
    c = CASES[name]
    kind, hyp, Y, w = c["kind"], c["hyp"], c["Y"], c["w"]
    Q = Y.shape[1]
    ctx.set_option(hipabi.OPT_FUSED_GRAM, fused_gram)
    try:
        _single(ctx, c["X"], Y[:, 0], c["mean"][0], kind, hyp)
        ctx.solve_targets(Y, c["mean"][None, :])
        worst = _check_moments(name, c, ctx.loo_targets())
        K = dk.d_hyper(kind, hyp[:-1], c["X"])[0]
        g, lpd = ctx.loo_targets_gradients(hyp.size, w[None, :])
        assert _same_bits(lpd, ctx.loo_targets()[2])
        worst = max(worst, _check(f"{name} weighted", g[0], c["wsum"], lcd.gradient_tolerance(c, c["grad"], w, K)))
        ones = np.ones(Q)
        worst = max(worst, _check(f"{name} ones", ctx.loo_targets_gradients(hyp.size)[0][0], lcd.weighted(c["grad"], ones),
                                  lcd.gradient_tolerance(c, c["grad"], ones, K)))
        for j in sorted({0, Q - 1}):
            e = _one_hot(Q, j)
            worst = max(worst, _check(f"{name} column {j}", ctx.loo_targets_gradients(hyp.size, e[None, :])[0][0], c["grad"][j],
                                      lcd.gradient_tolerance(c, c["grad"], e, K)))
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
    print(f"\n{name} fused_gram={fused_gram}: worst err/tol {worst:.3g}")


# ------------------------------------------------------------------------------------- (2) tile edges, column chunks, wide inputs

def _columns(seed, X, Q):
    rng = np.random.default_rng(seed)
    j = np.arange(Q)
    return (np.sin((1.0 + j)[None, :] * X[:, :1]) * (1.0 + 0.5 * j)[None, :] + 3.0 * (j % 3)[None, :]
            + 0.1 * rng.standard_normal((X.shape[0], Q)))


def _dense_case(kind, hyp, X, Y, mean):
    """A case in the fixture's layout with float64 references from the dense module (the literal form per column)."""
    mu, var, lpd = lcd.moments(kind, hyp, X, Y, mean)
    K = dk.d_hyper(kind, hyp[:-1], X)[0]
    ev = np.linalg.eigvalsh(K + (np.exp(2.0 * hyp[-1]) + lcd.JITTER) * np.eye(X.shape[0]))
    return dict(kind=kind, X=X, Y=Y, mean=np.asarray(mean, dtype=np.float64), hyp=hyp, mu=mu, var=var, lpd=lpd, kss=np.diag(K).copy(),
                cond=float(ev[-1] / ev[0]), weak=False, grad=lcd.column_gradients_literal(kind, hyp, X, Y, mean)), K


def _against_dense(ctx, tag, kind, hyp, X, Y, mean, w):
    c, K = _dense_case(kind, hyp, X, Y, mean)
    _single(ctx, X, Y[:, 0], mean[0], kind, hyp)
    ctx.solve_targets(Y, mean[None, :])
    _check_moments(tag, c, ctx.loo_targets(), 2.0)
    g, _ = ctx.loo_targets_gradients(hyp.size, w[None, :])
    _check(f"{tag} weighted", g[0], lcd.weighted(c["grad"], w), 2.0 * lcd.gradient_tolerance(c, c["grad"], w, K))
    # the M form of the dense module, which shares the algebra but none of the code
    _check(f"{tag} M form", g[0], lcd.weighted_gradient(kind, hyp, X, Y, mean, w), 2.0 * lcd.gradient_tolerance(c, c["grad"], w, K))


_H3 = {0: [np.log(0.4), 0.1], 3: list(np.log([0.8, 1.2, 1.6])) + [0.0], 8: list(np.log([0.5, 0.8, 0.6])) + [-0.1],
       10: list(np.log([0.5, 0.7, 0.9])) + [np.log(0.3), -0.1]}


@pytest.mark.parametrize("n,Q,kind", [(1, 1, 0), (127, 17, 0), (128, 16, 8), (129, 33, 3), (257, 3, 10), (257, 33, 0), (600, 17, 8),
                                      (600, 1, 0)])
def test_tile_edges_and_column_chunks_against_the_dense_reference(ctx, n, Q, kind):
    """n = 1, 127, 128, 129, 257 and 600 (more than GS = 4 tile rows: super-tile order and XCD dealing); Q = 1, 3, 16, 17, 33
    across the 16-column chunk; weights with zeros."""
    rng = np.random.default_rng(1000 + n + Q)
    X = np.asfortranarray(rng.uniform(size=(n, 3)))
    Y = _columns(n + Q, X, Q)
    mean = np.mean(Y, axis=0) + 0.05
    hyp = np.array(_H3[kind] + [np.log(0.2)])
    w = rng.uniform(0.0, 2.0, size=Q)
    if Q > 2:
        w[1] = 0.0
    _against_dense(ctx, f"n {n} Q {Q} kind {kind}", kind, hyp, X, Y, mean, w)


@pytest.mark.parametrize("kind,D", [(0, 36), (4, 40), (8, 40), (10, 40)])
def test_wide_inputs_against_the_dense_reference(ctx, kind, D):
    """D = 36, IsoSE: the epilogue that reads the coordinates from global memory; D = 40 for ArdSEProduct, ArdMatern52 and ArdRQ:
    the chunked staging.  n = 130, Q = 3."""
    n, Q = 130, 3
    rng = np.random.default_rng(400 + kind)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Y = _columns(kind, X, Q)
    mean = np.mean(Y, axis=0)
    ll = np.log(np.sqrt(D) * np.linspace(0.3, 0.6, D))
    h = {0: [np.log(0.3 * np.sqrt(D)), 0.1], 4: list(ll) + [0.0], 8: list(ll) + [0.1], 10: list(ll) + [np.log(2.0), 0.0]}[kind]
    _against_dense(ctx, f"kind {kind} D {D}", kind, np.array(h + [np.log(0.2)]), X, Y, mean, np.array([0.5, 0.0, 1.75]))


# ------------------------------------------------------------------------------------- (3), (4) the existing LOO path, columns

@pytest.mark.parametrize("kind", [0, 3, 8])
def test_agreement_with_loo_and_loo_gradients_after_refits(ctx, kind):
    """Q = 1 with Y = y, the leaf mean and weight 1 against dsmgp_loo / dsmgp_loo_gradients on the same fit: var to the bit, mu,
    lpd and the gradient within tolerance; then Y = [y_1 y_2 y_3] against three rounds of set_train(y_q) + fit + loo_gradients."""
    n, D, Q = 300, 3, 3
    rng = np.random.default_rng(31 + kind)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Y = _columns(50 + kind, X, Q)
    mean = np.mean(Y, axis=0)
    hyp = np.array(_H3[kind] + [np.log(0.2)])
    c, K = _dense_case(kind, hyp, X, Y, mean)
    G = np.zeros((Q, hyp.size))
    for q in range(Q):
        _single(ctx, X, Y[:, q], mean[q], kind, hyp)
        mu1, var1, lpd1 = ctx.loo()
        G[q], _ = (a[0] for a in ctx.loo_gradients(hyp.size))
        ctx.solve_targets(Y[:, q], mean[None, q:q + 1])
        mu, var, lpd = ctx.loo_targets()
        assert _same_bits(var, var1)
        tm, _, _, ts = lcd.moment_tolerances(c, q)
        _check(f"kind {kind} column {q} mu", mu[:, 0], mu1, 2.0 * tm)
        _check(f"kind {kind} column {q} lpd", lpd[0, 0], lpd1[0], 2.0 * ts)
        e = _one_hot(Q, q)
        _check(f"kind {kind} Q = 1, column {q}", ctx.loo_targets_gradients(hyp.size)[0][0], G[q],
               2.0 * lcd.gradient_tolerance(c, c["grad"], e, K))
    ctx.solve_targets(Y, mean[None, :])
    for w in [_one_hot(Q, q) for q in range(Q)] + [np.array([1.5, 2.0, 0.75]), np.array([1.0, 0.0, 1.0])]:
        _check(f"kind {kind} weights {w}", ctx.loo_targets_gradients(hyp.size, w[None, :])[0][0], lcd.weighted(G, w),
               2.0 * lcd.gradient_tolerance(c, c["grad"], w, K))


def test_a_column_does_not_depend_on_its_neighbours_to_the_bit(ctx):
    """Column j of mu and lpd at Q = 17 -- the other columns 1e3-scaled -- is the same bits as at Q = 1 with that column."""
    n, kind = 130, 8
    rng = np.random.default_rng(77)
    X = np.asfortranarray(rng.uniform(size=(n, 3)))
    col = _columns(9, X, 1)[:, 0]
    hyp = np.array(_H3[kind] + [np.log(0.2)])
    _single(ctx, X, col, 0.1, kind, hyp)
    ctx.solve_targets(col, np.array([[0.1]]))
    mu1, var1, lpd1 = ctx.loo_targets()
    for j in (0, 15, 16):
        Y = 1e3 * rng.standard_normal((n, 17))
        Y[:, j] = col
        mean = rng.standard_normal((1, 17))
        mean[0, j] = 0.1
        ctx.solve_targets(Y, mean)
        mu, var, lpd = ctx.loo_targets()
        assert _same_bits(mu[:, j], mu1[:, 0]) and _same_bits(lpd[0, j], lpd1[0, 0]) and _same_bits(var, var1), j


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
    W = np.random.default_rng(3).uniform(0.0, 2.0, size=(L, Q))
    W[5, 1] = 0.0
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
            out = [*ctx.loo_targets_gradients(stride, W), *ctx.loo_targets()]
            assert all(np.all(np.isfinite(a)) for a in out)
            again = [*ctx.loo_targets_gradients(stride, W), *ctx.loo_targets()]
            ctx.gradients(stride)                       # the gradient pass inverts again: the arena is rewritten in between
            third = [*ctx.loo_targets_gradients(stride, W), *ctx.loo_targets()]
            for a, b, d in zip(out, again, third):
                assert _same_bits(a, b) and _same_bits(a, d)
            res.append(out)
            fac.append(_factors(ctx))
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)
    same = [l for l in range(T["kid"].size) if _same_bits(fac[0][l], fac[1][l])]
    print(f"\nleaves whose factors are the same bits under one and two lanes: {len(same)} of {T['kid'].size}")
    assert same, "no leaf keeps its factor bits across lane counts: nothing to compare on"
    ptr = T["obs_ptr"]
    for l in same:
        rows = slice(int(ptr[l]), int(ptr[l + 1]))
        assert _same_bits(res[0][0][l], res[1][0][l]) and _same_bits(res[0][1][l], res[1][1][l]), l
        assert _same_bits(res[0][2][rows], res[1][2][rows]) and _same_bits(res[0][3][rows], res[1][3][rows]), l


# ------------------------------------------------------------------------------------- (6) every kind, COPY and PREFIX leaves

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
    """Kernel ids 0..10 = the eleven kinds in one leaf table, leaves of n = 2, 130 and 300 for each, COPY leaves with their
    source's mean row and with a mean row of their own, and a PREFIX leaf; targets, means and weights per (leaf, column), one
    leaf with a row of zero weights.  Every gradient row equals the same leaf alone in a context to 1e-12 relative (task dealing
    reorders the sums), and so do mu, var and lpd."""
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
    for s, own in ((2, False), (10, False), (26, True), (31, True)):
        obs.append(obs[s].copy())
        kid.append(kid[s])
        means.append(means[s] + (0.3 * np.arange(1, Q + 1) if own else 0.0))
        op.append(1)
        src.append(s)
        plen.append(0)
    s = 13
    obs.append(np.concatenate([obs[s], 2000 + np.sort(rng.choice(N - 2000, size=80, replace=False))]))
    kid.append(kid[s])
    means.append(np.mean(Y[obs[-1]], axis=0))
    op.append(2)
    src.append(s)
    plen.append(obs[s].size)
    L = len(obs)
    W = rng.uniform(0.0, 2.0, size=(L, Q))
    W[3, 2] = 0.0
    W[7] = 0.0                                                          # a leaf without weight: a row of zeros
    stride = D + 3

    def setup(c, leaves):
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
        full, lpd_full = mixed.loo_targets_gradients(stride, W)
        mu_full, var_full, lpd2 = mixed.loo_targets()
        assert _same_bits(lpd_full, lpd2)
    finally:
        mixed.close()
    ptr = np.concatenate([[0], np.cumsum([o.size for o in obs])])
    alone = np.zeros((L, stride))
    for i in range(L):
        setup(ctx, [i])
        _, info, _ = ctx.fit()
        assert info[0] == 0
        ctx.solve_targets(Y, means[i][None, :])
        alone[i] = ctx.loo_targets_gradients(stride, W[i:i + 1])[0][0]
        mu, var, lpd = ctx.loo_targets()
        for got, ref in ((mu_full[ptr[i]:ptr[i + 1]], mu), (var_full[ptr[i]:ptr[i + 1]], var), (lpd_full[i], lpd[0])):
            assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref)), i      # (the fit's schedule differs: not the same bits)
    assert np.all(full[7] == 0.0) and np.all(alone[7] == 0.0)
    scale = np.max(np.abs(alone), axis=1)
    scale[7] = 1.0
    assert np.all(scale > 0)
    rel = np.max(np.abs(full - alone), axis=1) / scale
    print(f"\n{L} leaves: worst relative difference {np.max(rel):.3g} (leaf {int(np.argmax(rel))})")
    assert np.all(rel <= 1e-12), (int(np.argmax(rel)), float(np.max(rel)))
    for i in range(L):
        assert np.all(full[i, len(_HYP[kid[i]]):] == 0.0)


# ------------------------------------------------------------------------------------- (7) non-interference

def test_nothing_else_moves(ctx):
    """fit's outputs, gradients, loo, loo_gradients, predict_fetch, predict_gradients, targets_fetch, predict_targets and
    targets_gradients, also under a set_gradient_leaves mask: the same bits before and after the two calls."""
    T = TABLE
    L = T["kid"].size
    Y, mean, W = _table_targets()
    stride = int(np.max(T["hyp_len"]))
    mask = np.arange(L) % 3 != 1

    def both():
        ctx.loo_targets()
        ctx.loo_targets_gradients(stride, W)

    def everything(call):
        _table_setup(ctx)
        out = list(ctx.fit()[:2])
        ctx.predict_run()
        ctx.solve_targets(Y, mean)
        if call:
            both()
        out += [ctx.gradients(stride), *ctx.loo_gradients(stride), *ctx.predict_fetch(), *ctx.loo(), ctx.predict_targets(),
                *ctx.predict_gradients(), ctx.targets_gradients(stride, W)]
        out += [ctx.targets_fetch(l) for l in (0, L - 1)]
        if call:
            both()
        ctx.set_gradient_leaves(mask)
        try:
            if call:
                both()
            masked = ctx.gradients(stride)
            assert np.all(masked[~mask] == 0.0)
            if call:
                assert np.all(np.any(ctx.loo_targets_gradients(stride, W)[0][~mask] != 0.0, axis=1))      # the mask does not apply
            out += [masked, ctx.gradients(stride), *ctx.loo_gradients(stride), *ctx.loo(), *ctx.predict_fetch(), ctx.targets_fetch(0),
                    ctx.targets_gradients(stride, W)]
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
    c = CASES["isose_n40_q3"]
    X, Y, n, hyp = c["X"], c["Y"], c["X"].shape[0], c["hyp"]
    dp = hipabi._dp
    ctx = hipabi.Context(0)
    try:
        ctx.set_train(X, Y[:, 0])
        ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
        ctx.set_hyper(0, 0, hyp)
        ctx.targets_Q = 3
        assert _code(lambda: ctx.loo_targets_gradients(3)) == hipabi.E_STATE        # no fit
        assert _code(ctx.loo_targets) == hipabi.E_STATE
        ctx.fit()
        assert _code(lambda: ctx.loo_targets_gradients(3)) == hipabi.E_STATE        # no solve_targets
        assert _code(ctx.loo_targets) == hipabi.E_STATE
        ctx.solve_targets(Y, np.zeros((1, 3)))
        ref, lpd = ctx.loo_targets_gradients(3)
        mu, var, lpd2 = ctx.loo_targets()
        assert _same_bits(lpd, lpd2)
        assert _code(lambda: ctx.loo_targets_gradients(2)) == hipabi.E_ARG          # stride smaller than the hyper-vector
        for bad in (np.nan, np.inf, -1e-300, -1.0):
            assert _code(lambda: ctx.loo_targets_gradients(3, np.array([[1.0, bad, 1.0]]))) == hipabi.E_ARG
        g = np.zeros((1, 3))
        assert ctx.lib.dsmgp_loo_columns_gradients(ctx.h, None, 3, None, None, None) == hipabi.E_ARG
        assert ctx.lib.dsmgp_loo_columns_gradients(ctx.h, g.ctypes.data_as(dp), 3, None, None, None) == 0   # lpd, seconds NULL
        assert _same_bits(g, ref) and ctx.loo_targets_gradients_seconds > 0.0 and ctx.loo_targets_seconds > 0.0
        assert ctx.lib.dsmgp_loo_columns(ctx.h, None, 0, None, None, None) == 0                              # every output NULL
        m = np.zeros((n, 3), order="F")
        assert ctx.lib.dsmgp_loo_columns(ctx.h, m.ctypes.data_as(dp), n - 1, None, None, None) == hipabi.E_ARG    # ld < obs_ptr[L]
        wide = np.zeros((n + 3, 3), order="F")
        assert ctx.lib.dsmgp_loo_columns(ctx.h, wide.ctypes.data_as(dp), n + 3, None, None, None) == 0
        assert _same_bits(wide[:n], mu) and np.all(wide[n:] == 0.0)
        g5, _ = ctx.loo_targets_gradients(5)
        assert _same_bits(g5[:, :3], ref) and np.all(g5[:, 3:] == 0.0)
        zero, _ = ctx.loo_targets_gradients(3, np.zeros((1, 3)))                     # a row of zero weights: zeros
        assert np.all(zero == 0.0)
        ctx.fit()                                                                    # a later fit: Z is stale
        assert _code(lambda: ctx.loo_targets_gradients(3)) == hipabi.E_STATE
        assert _code(ctx.loo_targets) == hipabi.E_STATE
        ctx.solve_targets(Y, np.zeros((1, 3)))
        assert _same_bits(ctx.loo_targets_gradients(3)[0], ref)                      # the context stays usable
        ctx.release()
        assert _code(lambda: ctx.loo_targets_gradients(3)) == hipabi.E_STATE
        ctx.fit()
        ctx.solve_targets(Y[:, :1], np.zeros((1, 1)))
        assert ctx.loo_targets_gradients(3)[0].shape == (1, 3) and ctx.loo_targets()[0].shape == (n, 1)
    finally:
        ctx.close()


def test_ardse_is_refused_above_the_staging_limit_whatever_the_option_says():
    n, D = 40, 36
    rng = np.random.default_rng(8)
    X = np.asfortranarray(rng.uniform(size=(n, D)))
    Y = _columns(8, X, 2)
    hyp = np.array(list(np.log(np.sqrt(D) * np.linspace(0.3, 0.6, D))) + [0.0, np.log(0.2)])
    ctx = hipabi.Context(0)
    try:
        _single(ctx, X, Y[:, 0], 0.0, 1, hyp)
        ctx.solve_targets(Y, np.zeros((1, 2)))
        for opt in (0, 1):
            ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, opt)
            assert _code(lambda: ctx.loo_targets_gradients(hyp.size)) == hipabi.E_ARG
            assert _code(lambda: ctx.loo_gradients(hyp.size)) == hipabi.E_ARG
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
        assert np.all(np.isfinite(ctx.loo_targets()[2]))                             # the moments have no such limit (dsmgp_loo's rule)
    finally:
        ctx.close()


def test_under_a_reserved_pool_the_same_bits(ctx):
    """With dsmgp_reserve H and U come from the pool's stack: the same bits as without a pool, also after a new test set has
    reset the stack above the plan (the arenas of the targets go with it) and after dsmgp_release."""
    n, Q, kind = 300, 17, 8
    rng = np.random.default_rng(12)
    X = np.asfortranarray(rng.uniform(size=(n, 3)))
    Y = _columns(12, X, Q)
    mean = np.mean(Y, axis=0)
    hyp = np.array(_H3[kind] + [np.log(0.2)])
    w = rng.uniform(0.0, 2.0, size=(1, Q))

    def both(c):
        return [*c.loo_targets_gradients(hyp.size, w), *c.loo_targets()]

    _single(ctx, X, Y[:, 0], mean[0], kind, hyp)
    ctx.solve_targets(Y, mean[None, :])
    ref = both(ctx)
    pooled = hipabi.Context(0)
    try:
        pooled.reserve(1 << 28)
        _single(pooled, X, Y[:, 0], mean[0], kind, hyp)
        assert _code(lambda: pooled.loo_targets_gradients(hyp.size)) == hipabi.E_STATE
        pooled.solve_targets(Y, mean[None, :])
        assert all(_same_bits(a, b) for a, b in zip(both(pooled), ref))
        pooled.set_test(X[:5], [0, 5], np.arange(5))            # the stack above the plan is reset
        assert _code(lambda: pooled.loo_targets_gradients(hyp.size)) == hipabi.E_STATE
        pooled.fit()
        pooled.solve_targets(Y, mean[None, :])
        assert all(_same_bits(a, b) for a, b in zip(both(pooled), ref))
        assert _same_bits(pooled.loo_gradients(hyp.size)[0], ctx.loo_gradients(hyp.size)[0])
        pooled.release()
        pooled.fit()
        pooled.solve_targets(Y, mean[None, :])
        assert all(_same_bits(a, b) for a, b in zip(both(pooled), ref))
    finally:
        pooled.close()


def test_failed_leaf_gets_nan_and_the_others_are_unaffected(ctx):
    """Leaf 0: a rank-1 linear Gram of size 1e16 (not positive definite in float64, as tests/test_targets_gpu.py builds it);
    leaf 1: an ordinary IsoSE leaf, which equals itself alone in a context to the bit."""
    n0, n1 = 140, 100
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Y = np.stack([y, np.cos(X[:, 0]) + 3.0], axis=1)
    mean = np.array([[0.0, 0.0], [0.2, 3.5]])
    W = np.array([[1.0, 1.0], [0.5, 2.0]])
    hyp1 = np.array([np.log(0.3), 0.0, np.log(0.1)])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, hyp1)
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    ctx.solve_targets(Y, mean)
    g, lpd = ctx.loo_targets_gradients(3, W)
    mu, var, lpd2 = ctx.loo_targets()
    assert np.all(np.isnan(g[0])) and np.all(np.isfinite(g[1])) and np.all(np.isnan(lpd[0])) and np.all(np.isfinite(lpd[1]))
    assert np.all(np.isnan(mu[:n0])) and np.all(np.isnan(var[:n0])) and np.all(np.isfinite(mu[n0:])) and np.all(np.isfinite(var[n0:]))
    assert _same_bits(lpd, lpd2)
    c, K = _dense_case(0, hyp1, X[n0:], Y[n0:], mean[1])
    _check("good leaf", g[1], lcd.weighted(c["grad"], W[1]), 2.0 * lcd.gradient_tolerance(c, c["grad"], W[1], K))
    alone = hipabi.Context(0)
    try:
        _single(alone, X[n0:], y[n0:], 0.2, 0, hyp1)
        alone.solve_targets(Y[n0:], mean[1:])
        ga, la = alone.loo_targets_gradients(3, W[1:])
        ma, va, _ = alone.loo_targets()
        assert _same_bits(ga[0], g[1]) and _same_bits(la[0], lpd[1]) and _same_bits(ma, mu[n0:]) and _same_bits(va, var[n0:])
    finally:
        alone.close()


# ------------------------------------------------------------------------------------- (9) the models

def _dense_objective_and_gradient(target, single, Y, means):
    """loo_targets_objective and its gradient from the dense module leaf by leaf -- the table of densities, the model's own
    recursion over it, the weighted dense gradients scattered the way grad_loo_targets scatters the device's rows -- with the
    tolerances of the leaves carried along: a table entry gets twice its column's loo_tol (both sides float64); the objective
    the sum of them (every node value moves by at most the sum of its leaves' errors); a leaf's row twice its
    gradient_tolerance at its weights, plus what the error dt of the table does to the weights themselves, W (exp(2 dt) - 1)
    times the size of the column's gradient."""
    from deepstructuredmixtures_amd import model as M
    L, Q = target.L, Y.shape[1]
    tab, ttab, cases = np.zeros((L, Q)), np.zeros((L, Q)), []
    for l, lf in enumerate(target.leaves):
        hyp = np.concatenate([lf.kernel.loghyp(), [lf.logNoise]])
        c, K = _dense_case(lf.kernel.kind, hyp, np.asfortranarray(target.x[lf.obs]), Y[lf.obs], means[l])
        cases.append((c, K))
        tab[l] = c["lpd"]
        ttab[l] = [2.0 * lcd.moment_tolerances(c, q)[3] for q in range(Q)]
    dt = float(np.sum(ttab))
    if single:
        W = np.ones((L, Q))
        obj = float(np.sum(tab[0]))
        visits = [(0, 1.0, 0, cases[0][0]["hyp"].size)]
    else:
        obj = float(sum(M._value_table(target, tab[:, q])[target.root.id] for q in range(Q)))
        W = np.zeros((L, Q))
        for q in range(Q):
            visits = M._tree_leaf_weights(target, M._value_table(target, tab[:, q]), None, rho=False)
            for leaf, w, _, _ in visits:
                W[leaf, q] += w
    rows = np.stack([lcd.weighted(c["grad"], W[l]) for l, (c, _) in enumerate(cases)])
    trow = np.stack([2.0 * lcd.gradient_tolerance(c, c["grad"], W[l], K)
                     + np.expm1(2.0 * dt) * np.sum(W[l][:, None] * np.abs(c["grad"]), axis=0) for l, (c, K) in enumerate(cases)])
    scatter = [(leaf, 1.0, off, size) for leaf, _, off, size in visits]
    if single:
        return tab, ttab, obj, dt, rows[0], trow[0]
    return tab, ttab, obj, dt, M._scatter_leaf_rows(target, rows, scatter), M._scatter_leaf_rows(target, trow, scatter)


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gp"])
def test_models_against_a_dense_loop(family):
    """A DSMGP, a PoE and a single GP: loo_targets, loo_targets_objective and grad_loo_targets against the dense module leaf by
    leaf, and three iterations of train(targets=Y, targets_objective="loo"), whose history starts at that objective."""
    import deepstructuredmixtures_amd as dsm
    from deepstructuredmixtures_amd.datagen import regression_data
    X, y, _ = regression_data(400, 2, n_test=1, seed=9400)
    Y = np.stack([y, np.sin(2.0 * X[:, 0]) + 0.1 * np.cos(7.0 * X[:, 1]), 0.5 * y + X[:, 1]], axis=1)
    kern = dict(kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.3))
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 2, 2, M=60, D=2, meanFun=dsm.ConstMean(float(np.mean(y))), **kern)
    elif family == "poe":
        m = dsm.buildPoE(X, y, 4, M=60, D=2, meanFun=dsm.ConstMean(float(np.mean(y))), **kern)
    else:
        X, y, Y = X[:150], y[:150], Y[:150]
        m = dsm.GaussianProcess(X, y, mean=dsm.ConstMean(float(np.mean(y))), **kern)
    target = m.model if family == "gp" else m
    dsm.fit(m)
    dsm.fit_targets(m, Y)
    means = dsm.targets_leaf_means(m, Y)
    tab, ttab, obj, tobj, grad, tgrad = _dense_objective_and_gradient(target, family == "gp", Y, means)
    res = dsm.loo_targets(m)
    assert res["lpd"].shape == (target.L, 3) and all(res["mu"][l].shape == (len(target.leaves[l].obs), 3) for l in range(target.L))
    _check(f"{family} lpd table", res["lpd"], tab, ttab)
    _check(f"{family} objective", dsm.loo_targets_objective(m), obj, tobj)
    _check(f"{family} gradient", dsm.grad_loo_targets(m), grad, tgrad)
    m, hist = dsm.train(m, dsm.ADAM(eta=0.01), randinit=False, iterations=3, targets=Y, targets_objective="loo")
    assert hist.size == 3 and np.all(np.isfinite(hist)) and abs(hist[0] - obj) <= tobj
    assert hist[-1] > hist[0]
    with pytest.raises(ValueError):
        dsm.train(m, iterations=1, targets=Y, targets_objective="elbo")
    with pytest.raises(ValueError):
        dsm.train(m, iterations=1, targets=Y, objective="loo")
