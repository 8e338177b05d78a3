"""GPU tests of dsmgp_kfold (csrc/kernels_kfold.hpp): k-fold cross-validation of every leaf GP from one fit, through
hipabi.Context.kfold, MultiContext.kfold and the model API.

References: tests/golden/gp_kfold.npz (50 digits from the definition, tests/golden/make_kfold_golden.py) for single leaves; for
the tile edges, the leaf table and the models a float64 reference formed in the test by tests/kfold_dense.py from
download_factor / kernel_matrix of the same context -- twice the tolerance there, both sides round.  Tolerances: kfold_dense
(pred_tolerance.moment_tol for the moments; for lpd 16 x the dense helper's recorded error against the fixture, the backward
bound of kfold_dense.lpd_tol_backward against the helper)."""
import math
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_kernels as dk
import kfold_dense as kd
import loo_dense
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel
from pred_tolerance import agg_tol, aggregate, mll_tol, moment_tol, row_entries

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = kd.load_cases()
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}
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
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    return float(mll[0])


def _isose(ctx, n, seed):
    X, y, _ = dsm.regression_data(n, 2, n_test=8, seed=seed)
    hyp, logNoise, mean = np.array([np.log(0.4), 0.0]), np.log(0.1), float(np.mean(y))
    mll = _single(ctx, X, y, mean, 0, hyp, logNoise)
    return X, y, hyp, logNoise, mean, mll


# ------------------------------------------------------------------------------------- (1) fixture cases

@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_against_50_digit_references(ctx, name):
    c = CASES[name]
    _single(ctx, c["X"], c["y"], c["mean"], c["kind"], c["loghyp"], c["logNoise"])
    mu, var, lpd, info = ctx.kfold(c["labels"], c["K"])
    n, K = c["y"].size, c["K"]
    assert mu.shape == (n,) and var.shape == (n,) and lpd.shape == (1, K) and info.shape == (1, K) and info.dtype == np.int32
    assert np.all(info == 0)
    held = c["labels"] >= 0
    assert np.array_equal(np.isnan(mu), ~held) and np.array_equal(np.isnan(var), ~held)
    tm, tv = kd.moment_tols(c["y"], c["mu"], c["var"], c["kss"], lib_noise(c["logNoise"]))
    m = np.array([np.sum(c["labels"] == k) for k in range(K)])
    tl = kd.lpd_tol_fixture(m, c["lpd_abs"], c["lpd_err_case"])
    print(f"\n{name}: lpd err {np.abs(lpd[0] - c['lpd'])}, dense helper's {c['lpd_err']} (case: {c['lpd_err_case']:.3g}), tol {tl}")
    _check(name + " mu", mu[held], c["mu"][held], tm[held])
    _check(name + " var", var[held], c["var"][held], tv[held])
    _check(name + " lpd", lpd[0], c["lpd"], tl)
    again = ctx.kfold(c["labels"], c["K"])
    assert all(_same_bits(p, q) for p, q in zip((mu, var, lpd), again[:3])) and np.array_equal(info, again[3])


# ------------------------------------------------------------------------------------- (2) tile edges

def test_tile_edges_n420(ctx):
    """Row tiles 128 / 128 / 128 / 36; blocks of exactly 1, 128, 129 and 162 rows.  The 162-row block is the last 162 positions
    (its first row is position 258, in the third tile: its K range starts late); the 129-row block holds positions 0 and 257."""
    n = 420
    X, y, hyp, logNoise, mean, _ = _isose(ctx, n, 420)
    labels = np.empty(n, dtype=np.int32)
    labels[258:] = 3
    labels[[0, 257]] = 2
    mid = np.arange(1, 257)
    perm = mid[np.argsort(dsm.datagen.uniform(77, 0, mid.size), kind="stable")]
    labels[perm[:127]] = 2
    labels[perm[127:255]] = 1
    labels[perm[255:]] = 0
    assert [int(np.sum(labels == k)) for k in range(4)] == [1, 128, 129, 162]
    mu, var, lpd, info = ctx.kfold(labels, 4)
    assert np.all(info == 0)
    F, _ = ctx.download_factor(0, n)
    kss = np.diag(ctx.kernel_matrix(0, X, X))
    r = kd.check_leaf(mu, var, lpd[0], F, y, mean, labels, 4, kss, lib_noise(logNoise))
    print(f"\ntile edges: err/tol mu {r[0]:.3g} var {r[1]:.3g} lpd {r[2]:.3g}")
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------------------------- (3) the two extremes

def test_one_fold_is_the_prior_and_singletons_are_loo(ctx):
    n = 300
    X, y, hyp, logNoise, mean, mll = _isose(ctx, n, 300)
    noise = lib_noise(logNoise)
    Kd = ctx.kernel_matrix(0, X, X)
    kss = np.diag(Kd)
    F, alpha = ctx.download_factor(0, n)
    cond, normK = kd.factor_stats(F)
    tb = kd.lpd_tol_backward(n, cond, alpha, normK)
    # K = 1: every row held out at once -- the prior predicts, and the joint density is the log marginal likelihood
    mu, var, lpd, info = ctx.kfold(np.zeros(n, dtype=np.int32), 1)
    assert info[0, 0] == 0
    tm, tv = kd.moment_tols(y, np.full(n, mean), kss + noise + kd.JITTER, kss, noise)
    _check("K=1 mu = mean", mu, np.full(n, mean), 2.0 * tm)
    _check("K=1 var = diag K_y", var, kss + noise + kd.JITTER, 2.0 * tv)
    _check("K=1 lpd = mll", lpd[0, 0], mll, mll_tol(mll, cond) + tb)
    # K = n singletons: leave-one-out
    lm, lv, ll = ctx.loo()
    mu, var, lpd, info = ctx.kfold(np.arange(n, dtype=np.int32), n)
    assert np.all(info == 0) and lpd.shape == (1, n)
    tm, tv, _, ts = loo_dense.loo_tol(y, lm, lv, kss, noise)
    _check("singletons mu = loo", mu, lm, 2.0 * tm)
    _check("singletons var = loo", var, lv, 2.0 * tv)
    _check("singletons sum lpd = loo", np.sum(lpd[0]), ll[0], 2.0 * ts)


# ------------------------------------------------------------------------------------- (4) the leaf table

def _table_setup(ctx, mean=None):
    T = TABLE
    ctx.set_train(T["X"], T["y"])
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean"] if mean is None else mean)
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])


def _table_labels(K=4):
    """Per-row random labels 0 .. K - 2, and label K - 1 on three rows of leaf 5 only: most leaves have no row of it."""
    T = TABLE
    N = T["X"].shape[0]
    labels = np.minimum((dsm.datagen.uniform(41, 0, N) * (K - 1)).astype(np.int32), K - 2)
    a = int(T["obs_ptr"][5])
    labels[T["obs_idx"][a:a + 3]] = K - 1
    return labels.astype(np.int32)


def _table_check(ctx, tag, mean, labels, K, got, factor=2.0):
    T = TABLE
    op_, ob = T["obs_ptr"], T["obs_idx"]
    mu, var, lpd, info = got
    worst, empty = 0.0, 0
    for l in range(T["kid"].size):
        a, b = int(op_[l]), int(op_[l + 1])
        rows = ob[a:b]
        kid = int(T["kid"][l])
        noise = lib_noise(T["hyp"][kid][T["hyp_len"][kid] - 1])
        F, _ = ctx.download_factor(l, b - a)
        Xl = np.asfortranarray(T["X"][rows])
        kss = np.diag(ctx.kernel_matrix(kid, Xl, Xl))
        r = kd.check_leaf(mu[a:b], var[a:b], lpd[l], F, T["y"][rows], float(mean[l]), labels[rows], K, kss, noise, factor)
        assert max(r) <= 1.0, (tag, l, r)
        assert np.all(info[l] == 0)
        for k in range(K):
            if not np.any(labels[rows] == k):
                assert lpd[l, k] == 0.0 and info[l, k] == 0
                empty += 1
        worst = max(worst, max(r))
    assert empty > 0
    print(f"\n{tag}: {T['kid'].size} leaves, {empty} empty blocks, worst err/tol {worst:.3g}")


def test_leaf_table_with_copy_and_prefix_leaves_and_lanes(ctx):
    T = TABLE
    K = 4
    labels = _table_labels(K)
    assert T["op"][CPY] == 1 and T["src"][CPY] == SRC and T["op"][PRE] == 2 and T["mean"][CPY] == T["mean"][SRC]
    a, b = (int(v) for v in T["obs_ptr"][CPY:CPY + 2])
    s0, s1 = (int(v) for v in T["obs_ptr"][SRC:SRC + 2])
    got = {}
    try:
        for lanes in (1, 2):
            ctx.set_option(hipabi.OPT_LANES, lanes)
            _table_setup(ctx)
            _, info, _ = ctx.fit()
            assert np.all(info == 0) and ctx.lanes() == lanes
            got[lanes] = ctx.kfold(labels, K)
            _table_check(ctx, f"table lanes={lanes}", T["mean"], labels, K, got[lanes])
        # per-leaf results do not depend on the lane (test_loo_gpu.test_lanes_and_step_kinds_agree): the same bits
        assert all(_same_bits(p, q) for p, q in zip(got[1][:3], got[2][:3])) and np.array_equal(got[1][3], got[2][3])
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)
    same = got[1]
    # the COPY leaf with its source's mean: its source's alpha, the source's bits
    assert _same_bits(same[0][a:b], same[0][s0:s1]) and _same_bits(same[1][a:b], same[1][s0:s1])
    assert _same_bits(same[2][CPY], same[2][SRC])
    mean2 = T["mean"].copy()
    mean2[CPY] += 0.37
    ctx.set_option(hipabi.OPT_LANES, 1)
    try:
        _table_setup(ctx, mean2)
        _, info, _ = ctx.fit()
        assert np.all(info == 0)
        other = ctx.kfold(labels, K)
        _table_check(ctx, "table, COPY leaf with another mean", mean2, labels, K, other)
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)
    assert _same_bits(other[1][a:b], same[1][a:b])                  # the variances do not see the mean
    assert not _same_bits(other[0][a:b], same[0][a:b]) and not _same_bits(other[2][CPY], same[2][CPY])
    keep = np.ones(same[0].size, dtype=bool)
    keep[a:b] = False
    assert _same_bits(other[0][keep], same[0][keep]) and _same_bits(other[1][keep], same[1][keep])


# ------------------------------------------------------------------------------------- (5) relabelling

def test_results_depend_on_the_row_sets_only(ctx):
    T = TABLE
    K = 4
    labels = _table_labels(K)
    _table_setup(ctx)
    ctx.fit()
    mu, var, lpd, info = ctx.kfold(labels, K)
    perm = np.array([2, 0, 3, 1], dtype=np.int32)           # old label k becomes perm[k]
    mu2, var2, lpd2, info2 = ctx.kfold(perm[labels], K)
    assert _same_bits(mu, mu2) and _same_bits(var, var2)
    assert _same_bits(lpd, lpd2[:, perm]) and np.array_equal(info, info2[:, perm])
    # other labels (and another K) on the rows outside leaf 7: nothing of leaf 7 moves
    l0 = 7
    a, b = int(T["obs_ptr"][l0]), int(T["obs_ptr"][l0 + 1])
    inside = np.zeros(labels.size, dtype=bool)
    inside[T["obs_idx"][a:b]] = True
    lab3 = np.where(inside, labels, (labels + 1 + np.arange(labels.size) % 3) % 6).astype(np.int32)
    mu3, var3, lpd3, _ = ctx.kfold(lab3, 6)
    assert _same_bits(mu[a:b], mu3[a:b]) and _same_bits(var[a:b], var3[a:b]) and _same_bits(lpd[l0], lpd3[l0, :K])
    assert not _same_bits(mu, mu3)


# ------------------------------------------------------------------------------------- (6) the neighbours keep their bits

def test_neighbours_keep_their_bits(ctx):
    T = TABLE
    L = T["kid"].size
    K = 4
    labels = _table_labels(K)
    stride = int(np.max(T["hyp_len"]))
    nt = 24
    Xt = np.asfortranarray(T["X"][:nt] + 0.01)
    rptr = np.arange(L + 1, dtype=np.int64) * nt
    ridx = np.tile(np.arange(nt, dtype=np.int64), L)
    eps = dsm.datagen.normal(9, 0, L * nt * 2).reshape((L * nt, 2), order="F")
    _table_setup(ctx)
    ctx.set_test(Xt, rptr, ridx)
    mll0, info0, _ = ctx.fit()
    ctx.predict_run()
    before = dict(loo=ctx.loo(), pred=ctx.predict_fetch(), draw=ctx.predict_sample(eps)[0], grad=ctx.gradients(stride))
    ctx.loo()                                               # (the gradient pass inverts on every call: L^-T of loo again)
    got = ctx.kfold(labels, K)
    assert ctx.kfold_split_seconds[0] == 0.0 and ctx.kfold_seconds > 0.0        # L^-T as loo left it
    after = dict(loo=ctx.loo(), pred=ctx.predict_fetch(), draw=ctx.predict_sample(eps)[0], grad=ctx.gradients(stride))
    for k in before:
        p, q = before[k], after[k]
        assert all(_same_bits(x, z) for x, z in zip(p, q)) if isinstance(p, tuple) else _same_bits(p, q), k
    mll1, info1, _ = ctx.fit()
    assert _same_bits(mll0, mll1) and np.array_equal(info0, info1)
    fresh = ctx.kfold(labels, K)                            # first after a fit: the inversion runs here
    assert ctx.kfold_split_seconds[0] > 0.0
    assert all(_same_bits(p, q) for p, q in zip(got[:3], fresh[:3]))
    mask = np.zeros(L, dtype=np.int32)
    mask[[3, 7, CPY]] = 1
    try:
        ctx.set_gradient_leaves(mask)
        ctx.fit()
        g_mask = ctx.gradients(stride)
        masked = ctx.kfold(labels, K)                       # the mask does not apply
        assert all(_same_bits(p, q) for p, q in zip(got[:3], masked[:3]))
        assert _same_bits(g_mask, ctx.gradients(stride))
    finally:
        ctx.set_gradient_leaves(None)


# ------------------------------------------------------------------------------------- (7) a failed leaf

def test_failed_leaf_gets_nan_and_the_others_are_unaffected(ctx):
    """test_loo_gpu's construction: leaf 0 a rank-1 linear Gram of size 1e16 (not positive definite), leaf 1 an IsoSE leaf."""
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
    labels = (np.arange(n0 + n1) % 3).astype(np.int32)
    mu, var, lpd, kinfo = ctx.kfold(labels, 3)
    assert np.all(np.isnan(mu[:n0])) and np.all(np.isnan(var[:n0])) and np.all(np.isnan(lpd[0])) and np.all(kinfo[0] == -1)
    assert np.all(kinfo[1] == 0)
    Kd = dk.value(0, hyp1, X[n0:], X[n0:])
    noise = lib_noise(np.log(0.1))
    F, _ = ctx.download_factor(1, n1)
    r = kd.check_leaf(mu[n0:], var[n0:], lpd[1], F, y[n0:], 0.2, labels[n0:], 3, np.diag(Kd), noise)
    print(f"\ngood leaf: err/tol {r}")
    assert max(r) <= 1.0, r


# ------------------------------------------------------------------------------------- (8) refusals, NULL outputs, memory

def test_errors_null_outputs_and_no_inverse_without_variances():
    c = CASES["isose_n127_k3"]
    n, K = c["y"].size, 3
    ctx = hipabi.Context(0)
    try:
        lib, dp, ip = ctx.lib, hipabi._dp, hipabi._ip
        lab = np.ascontiguousarray(c["labels"], dtype=np.int32)
        plab = lab.ctypes.data_as(ip)
        assert lib.dsmgp_kfold(None, plab, K, None, None, None, None, None) == hipabi.E_ARG
        ctx.set_train(c["X"], c["y"])
        ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
        ctx.set_hyper(0, c["kind"], np.concatenate([c["loghyp"], [c["logNoise"]]]))
        with pytest.raises(hipabi.DsmgpError) as e:         # before fit
            ctx.kfold(lab, K)
        assert e.value.code == hipabi.E_STATE
        ctx.fit()
        for bad_lab, bad_K in ((lab, 0), (lab, 2), (np.where(lab == 0, -2, lab), K), (lab, 65536)):
            with pytest.raises(hipabi.DsmgpError) as e:     # K = 0, a label equal to K, a label of -2, K too large
                ctx.kfold(bad_lab, bad_K)
            assert e.value.code == hipabi.E_ARG
        assert lib.dsmgp_kfold(ctx.h, None, K, None, None, None, None, None) == hipabi.E_ARG        # fold = NULL
        mu_only = ctx.kfold(lab, K, want_var=False)
        mu, var, lpd, info = ctx.kfold(lab, K)
        assert mu_only[1] is None and _same_bits(mu_only[0], mu) and _same_bits(mu_only[2], lpd)
        assert lib.dsmgp_kfold(ctx.h, plab, K, None, None, None, None, None) == 0                    # every output may be NULL
        m2, v2, l2, i2 = np.empty(n), np.empty(n), np.empty((1, K), order="F"), np.empty((1, K), dtype=np.int32, order="F")
        assert lib.dsmgp_kfold(ctx.h, plab, K, m2.ctypes.data_as(dp), None, None, None, None) == 0
        assert lib.dsmgp_kfold(ctx.h, plab, K, None, v2.ctypes.data_as(dp), None, None, None) == 0
        assert lib.dsmgp_kfold(ctx.h, plab, K, None, None, l2.ctypes.data_as(dp), None, None) == 0
        assert lib.dsmgp_kfold(ctx.h, plab, K, None, None, None, i2.ctypes.data_as(ip), None) == 0
        assert _same_bits(mu, m2) and _same_bits(var, v2) and _same_bits(lpd, l2) and np.array_equal(info, i2)
        ctx.set_hyper(0, c["kind"], np.concatenate([c["loghyp"] + 0.1, [c["logNoise"]]]))
        with pytest.raises(hipabi.DsmgpError) as e:         # new hyper-parameters: no fit yet
            ctx.kfold(lab, K)
        assert e.value.code == hipabi.E_STATE
        ctx.fit()
        assert not _same_bits(mu, ctx.kfold(lab, K)[0])
        ctx.release()
        with pytest.raises(hipabi.DsmgpError) as e:         # after release
            ctx.kfold(lab, K)
        assert e.value.code == hipabi.E_STATE
    finally:
        ctx.close()
    # one block of 1000 rows (mpad = 1024): the inverse factors are 8 MiB that only a call with variances allocates
    ctx = hipabi.Context(0)
    try:
        X, y, _ = dsm.regression_data(1000, 2, n_test=8, seed=1000)
        _single(ctx, X, y, float(np.mean(y)), 0, np.array([np.log(0.4), 0.0]), np.log(0.1))
        one = np.zeros(1000, dtype=np.int32)
        assert set(ctx.kfold_stats().values()) == {0}
        ctx.kfold(one, 1, want_var=False)
        st = ctx.kfold_stats()
        assert st["inverse_factors"] == 0 and st["factors"] == 1024 * 1024 * 8 and st["packed"] == 1024 * 1024 * 8
        ctx.kfold(one, 1)
        st2 = ctx.kfold_stats()
        assert st2["inverse_factors"] == 1024 * 1024 * 8 and {k: v for k, v in st2.items() if k != "inverse_factors"} == \
            {k: v for k, v in st.items() if k != "inverse_factors"}
        with pytest.raises(ValueError):                     # one label per training row
            ctx.kfold(one[:-1], 1)
        ctx.release()
        assert set(ctx.kfold_stats().values()) == {0}
    finally:
        ctx.close()
    sc = hipabi.StreamingContext(0)
    try:
        with pytest.raises(hipabi.DsmgpError) as e:
            sc.kfold(lab, K)
        assert e.value.code == hipabi.E_STATE
    finally:
        sc.close()


# ------------------------------------------------------------------------------------- (9) the model API, MultiContext

def _build(family, X, y):
    kern = dsm.IsoSE(np.log(0.3), 0.0)
    if family == "dsmgp":
        return dsm.buildDSMGP(X, y, 2, 3, M=40, kernel=kern, logNoise=np.log(0.1), seed=1)
    mean = dsm.ConstMean(float(np.mean(y)))
    if family in ("poe", "gpoe"):
        return dsm.buildPoE(X, y, 3, M=40, kernel=kern, meanFun=mean, logNoise=np.log(0.1), seed=1, generalized=family == "gpoe")
    return dsm.buildBCM(X, y, 3, M=40, kernel=kern, meanFun=mean, logNoise=np.log(0.1), seed=1, robust=True)


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gpoe", "rbcm"])
def test_model_kfold_predict_and_scores(family):
    """kfold_predict with singleton labels against loo_predict; with K = 3 against the same substitution done here with dense
    held-out moments (from the downloaded factors) and pred_tolerance.aggregate, tolerances carried through agg_tol."""
    X, y, _ = dsm.regression_data(420, 2, n_test=8, seed=99)
    model = _build(family, X, y)
    try:
        n = X.shape[0]
        noise = lib_noise(model.leaves[0].logNoise)
        kss1 = math.exp(2.0 * model.leaves[0].kernel.logs)
        yscale = max(1.0, float(np.max(np.abs(y))))
        lmu, lvar = dsm.loo_predict(model)
        smu, svar = dsm.kfold_predict(model, np.arange(n, dtype=np.int32))
        tm, tv = moment_tol(lmu, lvar, np.full(n, kss1), noise, yscale)
        _check(f"{family} singletons mu = loo_predict", smu, lmu, 4.0 * tm)
        _check(f"{family} singletons var = loo_predict", svar, lvar, 4.0 * tv)
        fold = dsm.make_folds(n, 3, seed=5)
        fold[::17] = -1
        res = dsm.kfold(model, fold)
        assert res["lpd"].shape == (model.L, 3) and np.all(res["info"] == 0)
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
            r = kd.check_leaf(res["mu"][l], res["var"][l], res["lpd"][l], F, y[obs], lf.mean.m, fold[obs], 3,
                              np.full(obs.size, kss1), noise)
            assert max(r) <= 1.0, (l, r)
            rm, rv, _ = kd.kfold_from_factor(F, y[obs], lf.mean.m, fold[obs], 3)
            tm, tv = kd.moment_tols(y[obs], rm, rv, np.full(obs.size, kss1), noise)
            where = {int(r_): i for i, r_ in enumerate(obs) if fold[r_] >= 0}
            for e in range(int(ptr[l]), int(ptr[l + 1])):
                i = where.get(int(idx[e]))
                if i is not None:
                    ref_mu[e], ref_var[e], tm_e[e], tv_e[e] = rm[i], rv[i], 2.0 * tm[i], 2.0 * tv[i]
                    nsub += 1
        assert nsub > 0
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
        mu, var = dsm.kfold_predict(model, fold)
        _check(f"{family} kfold_predict mu", mu, am, tm)
        _check(f"{family} kfold_predict var", var, av, tv)
        plain_mu, _ = dsm.predict(model, model.x)
        unheld = fold < 0
        assert np.max(np.abs(plain_mu - mu)[~unheld]) > 1e-6 and np.max(np.abs(plain_mu - mu)[unheld]) < 1e-9
        sc = dsm.kfold_scores(model, fold)
        held = ~unheld
        assert abs(sc["mse"] - dsm.mse(y[held], mu[held])) <= 1e-12 * max(1.0, sc["mse"]) and np.isfinite(sc["nlpd"])
    finally:
        model.ctx.close()


def test_multicontext_puts_the_leaves_back_in_table_order(ctx):
    T = TABLE
    K = 4
    labels = _table_labels(K)
    _table_setup(ctx)
    _, info, _ = ctx.fit()
    assert np.all(info == 0)
    one = ctx.kfold(labels, K)
    mc = hipabi.MultiContext(0, 2)
    try:
        _table_setup(mc)
        _, info, _ = mc.fit()
        assert np.all(info == 0) and len(mc.act) == 2
        two = mc.kfold(labels, K)
        assert mc.kfold_seconds > 0.0 and mc.kfold_split_seconds.shape == (4,)
    finally:
        mc.close()
    assert all(p.shape == q.shape for p, q in zip(one, two))
    _table_check(ctx, "table, two sub-contexts", T["mean"], labels, K, two)
    print(f"same bits as one context: {[_same_bits(p, q) for p, q in zip(one[:3], two[:3])]}")
