"""GPU tests of dsmgp_predict_cov: the full predictive covariance of a leaf, Sigma = K_tt - V'V (+ noise I)
(prediction(gp, xtest) of the reference, src/gaussianprocess.jl:110-137), from tile_predcov_kernel.

References: tests/golden/gp_predcov.npz (50 digits, tests/golden/make_predcov_golden.py) for single leaves of every kernel
kind; for leaf tables and the larger single GP a float64 reference formed in the test from download_factor and kernel_matrix
of the same context.  Tolerance per entry: the variance tolerance of pred_tolerance.moment_tol,
RTOL |Sigma_rc| + ATOL max(1, max(kss_r, kss_c) + noise) -- sigma^2 is the r = c case of the same difference k - v_r.v_c, and
|v_r.v_c| <= sqrt(kss_r kss_c) <= max(kss_r, kss_c) (Cauchy-Schwarz); twice that where both sides carry float64 rounding."""
import math
import os

import numpy as np
import pytest
import scipy.linalg as sla

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi
from pred_tolerance import ATOL, EPS, RTOL, moment_tol

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _load():
    z = np.load(os.path.join(GOLDEN, "gp_predcov.npz"))
    cases = {}
    for key in z.files:
        if "/" in key:
            name, field = key.split("/")
            cases.setdefault(name, {})[field] = z[key]
    for c in cases.values():        # meta = kind, mean, logNoise, cond, the pair of the row listed twice
        m = c.pop("meta")
        c.update(kind=int(m[0]), mean=float(m[1]), logNoise=float(m[2]), cond=float(m[3]), dup=(int(m[4]), int(m[5])))
    return cases


CASES = _load()
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}


def packed_lower(nt):
    """(rows, columns) of the fixture's packed lower triangle: column by column (make_predcov_golden.packed_lower)."""
    c, r = np.triu_indices(nt)
    return r, c


def entry_tol(S, kss, noise):
    kss = np.asarray(kss, dtype=np.float64)
    return RTOL * np.abs(S) + ATOL * np.maximum(1.0, np.maximum(kss[:, None], kss[None, :]) + noise)


def lib_noise(logNoise):
    """exp(2 logNoise) as the library forms it (std::exp of the doubled value: the C library's exp, as math.exp)."""
    return math.exp(2.0 * float(logNoise))


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _check(tag, got, ref, tol):
    """Every element within its tolerance; prints the worst error and error / tolerance."""
    got, ref, tol = (np.asarray(a, dtype=np.float64) for a in (got, ref, tol))
    err = np.abs(got - ref)
    ratio = err / tol
    worst = int(np.argmax(ratio)) if ratio.size else 0
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    assert np.all(err <= tol), (tag, worst, got.flat[worst], ref.flat[worst], tol.flat[worst])


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _single(ctx, c, path):
    """Fit + predict one fixture leaf; returns (mu, var) with the context left ready for predict_cov."""
    X, y, Xt = c["X"], c["y"], c["Xt"]
    n, nt = X.shape[0], Xt.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(c["mean"])])
    ctx.set_hyper(0, int(c["kind"]), np.concatenate([c["loghyp"], [float(c["logNoise"])]]))
    if path == "joint":
        ctx.set_test(Xt, [0, nt], np.arange(nt))
        _, info, _ = ctx.fit()
        ctx.predict_run()
        mu, var = ctx.predict_fetch()
    else:
        _, info, _ = ctx.fit()
        mu, var = ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
    assert info[0] == 0
    return mu, var


# ------------------------------------------------------------------------------------- (1)-(3) fixture cases

@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_covariance_against_50_digit_references(ctx, name, path):
    """Every fixture case by the standalone sweep and jointly, with and without noise, against the 50-digit Sigma; then the
    exact properties (symmetry, noise only on the diagonal and added once, the row listed twice, repeatability) on bits, and
    the consistency with predict_fetch's variances and, for the far rows of the SE-like kinds, with kernel_matrix."""
    c = CASES[name]
    Xt = c["Xt"]
    nt = Xt.shape[0]
    noise = lib_noise(c["logNoise"])
    kss = c["kss"]
    r, cc = packed_lower(nt)
    ref = np.zeros((nt, nt))
    ref[r, cc] = c["sigma"]
    ref[cc, r] = c["sigma"]
    mu, var = _single(ctx, c, path)
    S0 = ctx.predict_cov(0, nt, with_noise=False)
    S1 = ctx.predict_cov(0, nt, with_noise=True)
    assert S0.shape == (nt, nt) and S0.flags.f_contiguous
    tag = f"{name} {path}"
    # 1. against 50 digits
    _check(tag + " Sigma", S0, ref, entry_tol(ref, kss, noise))
    _check(tag + " Sigma + noise", S1, ref + noise * np.eye(nt), entry_tol(ref + noise * np.eye(nt), kss, noise))
    # 2. exact properties
    assert _same_bits(S0, S0.T) and _same_bits(S1, S1.T)
    off = ~np.eye(nt, dtype=bool)
    assert _same_bits(S0[off], S1[off])
    assert _same_bits(np.diag(S1), np.diag(S0) + noise)
    d0, d1 = (int(i) for i in c["dup"])
    assert _same_bits(S0[d0], S0[d1]) and _same_bits(S0[:, d0], S0[:, d1])
    assert _same_bits(S0, ctx.predict_cov(0, nt, with_noise=False)) and _same_bits(S1, ctx.predict_cov(0, nt, with_noise=True))
    # 3. the diagonal against predict_fetch (not bitwise: the sweep adds its sums of squares in block-step order)
    tv = moment_tol(var, var, kss, noise, 1.0)[1]
    _check(tag + " diag vs var", np.diag(S1), var, 2.0 * tv)
    K = ctx.kernel_matrix(0, Xt, Xt)
    if int(c["kind"]) not in (2, 3) and nt > 4:       # rows at +-1e3: k* underflows to 0, Sigma_rc = k(x*_r, x*_c)
        far = [i for i in range(nt) if abs(Xt[i, 0]) == 1e3]
        assert len(far) == 2
        for p in far:
            assert np.all(np.abs(S0[p] - K[p]) <= 16 * EPS * kss[p]), (p, np.max(np.abs(S0[p] - K[p])))


# ------------------------------------------------------------------------------------- (4) a leaf table

def _factor_reference(ctx, leaf, kid, Xl, Xr):
    F, _ = ctx.download_factor(leaf, Xl.shape[0])
    Knt = ctx.kernel_matrix(kid, Xl, Xr)
    V = sla.solve_triangular(np.tril(F), Knt, lower=True)
    Ktt = ctx.kernel_matrix(kid, Xr, Xr)
    return Ktt - V.T @ V, np.diag(Ktt).copy()


def _table_setup(ctx):
    T = TABLE
    ctx.set_train(T["X"], T["y"])
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean"])
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("fused_steps", [1, 0])
@pytest.mark.parametrize("path", ["joint", "standalone"])
def test_leaf_table_covariances(ctx, path, fused_steps, lanes):
    """The 41-leaf table of gp_pred.npz (a COPY and a PREFIX leaf, a leaf without routed rows, four kernel ids, 10 .. 150
    routed rows) with one or two lanes and the shallow steps fused or not: Sigma of every leaf against K_tt - V'V formed from
    download_factor and kernel_matrix of the same context, within twice the tolerance (both sides carry float64 rounding)."""
    T = TABLE
    L = T["kid"].size
    rp, ri, op_, ob = T["route_ptr"], T["route_idx"], T["obs_ptr"], T["obs_idx"]
    ctx.set_option(hipabi.OPT_FUSED_STEPS, fused_steps)
    ctx.set_option(hipabi.OPT_LANES, lanes)
    try:
        _table_setup(ctx)
        if path == "joint":
            ctx.set_test(T["Xt"], rp, ri)
            _, info, _ = ctx.fit()
            ctx.predict_run()
        else:
            _, info, _ = ctx.fit()
            ctx.predict_leaves(T["Xt"], rp, ri)
        assert np.all(info == 0) and ctx.lanes() == lanes
        leaves = range(L)
        got = {}
        for l in leaves:
            nt = int(rp[l + 1] - rp[l])
            got[l] = ctx.predict_cov(l, nt, with_noise=False)
            assert got[l].shape == (nt, nt)
        assert got[40].size == 0
        worst = 0.0
        for l in leaves:
            if got[l].size == 0:
                continue
            kid = int(T["kid"][l])
            noise = lib_noise(T["hyp"][kid][T["hyp_len"][kid] - 1])
            Xl = np.asfortranarray(T["X"][ob[op_[l]:op_[l + 1]]])
            Xr = np.asfortranarray(T["Xt"][ri[rp[l]:rp[l + 1]]])
            ref, kss = _factor_reference(ctx, l, kid, Xl, Xr)
            tol = 2.0 * entry_tol(ref, kss, noise)
            err = np.abs(got[l] - ref)
            worst = max(worst, float(np.max(err / tol)))
            assert np.all(err <= tol), (l, float(np.max(err / tol)))
            assert _same_bits(got[l], got[l].T)
        print(f"\ntable {path} fused_steps={fused_steps} lanes={lanes}: {len(got)} leaves, worst err/tol {worst:.3g}")
        # the COPY leaf shares its source's factor but sweeps its own rows: where the routed rows coincide, agreement within
        # the tolerance (not equal bits: the rows sit at other positions of other tiles, possibly in the other lane)
        src, cpy = 0, 32
        rs, rc = ri[rp[src]:rp[src + 1]], ri[rp[cpy]:rp[cpy + 1]]
        common, ia, ib = np.intersect1d(rs, rc, return_indices=True)
        if common.size:
            A, B = got[src][np.ix_(ia, ia)], got[cpy][np.ix_(ib, ib)]
            kid = int(T["kid"][src])
            kss = np.diag(ctx.kernel_matrix(kid, np.asfortranarray(T["Xt"][common]), np.asfortranarray(T["Xt"][common])))
            assert np.all(np.abs(A - B) <= entry_tol(A, kss, lib_noise(T["hyp"][kid][T["hyp_len"][kid] - 1])))
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)


# ------------------------------------------------------------------------------------- (5) a larger single GP

@pytest.mark.parametrize("path", ["standalone", "joint"])
def test_larger_single_gp(ctx, path):
    """n = 1500, nt = 400, D = 8, IsoSE: interior tiles of a 4 x 4 tile grid, K = 1496 + 4 tail columns."""
    n, nt, D = 1500, 400, 8
    X, y, Xt = dsm.regression_data(n, D, n_test=nt, seed=777)
    hyp = np.array([np.log(0.9), 0.0, np.log(0.1)])
    c = dict(X=X, y=y, Xt=Xt, mean=float(np.mean(y)), kind=0, loghyp=hyp[:2], logNoise=hyp[2])
    _single(ctx, c, path)
    S = ctx.predict_cov(0, nt, with_noise=False)
    ref, kss = _factor_reference(ctx, 0, 0, X, Xt)
    _check(f"n1500 {path}", S, ref, entry_tol(ref, kss, lib_noise(hyp[2])))
    assert _same_bits(S, S.T)
    print(f"predict_cov device seconds {ctx.cov_seconds:.3g}")


# ------------------------------------------------------------------------------------- (6) errors

def test_errors_leave_the_context_usable(ctx):
    c = CASES["isose_small"]
    X, y, Xt = c["X"], c["y"], c["Xt"]
    n, nt = X.shape[0], Xt.shape[0]
    hyp = np.concatenate([c["loghyp"], [float(c["logNoise"])]])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(c["mean"])])
    ctx.set_hyper(0, 0, hyp)
    ctx.fit()
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    with pytest.raises(hipabi.DsmgpError) as e:         # before predict_run
        ctx.predict_cov(0, nt)
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    S = ctx.predict_cov(0, nt)
    for leaf, m in ((1, nt), (-1, nt), (0, nt - 1)):      # bad leaf, ld < nt
        with pytest.raises(hipabi.DsmgpError) as e:
            ctx.predict_cov(leaf, m)
        assert e.value.code == hipabi.E_ARG
        assert _same_bits(S, ctx.predict_cov(0, nt))
    hyp2 = hyp.copy()
    hyp2[0] += 0.1
    ctx.set_hyper(0, 0, hyp2)
    ctx.fit()                                           # joint: the rows rode along, but predict_run has not finished them
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.predict_cov(0, nt)
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    S2 = ctx.predict_cov(0, nt)
    assert not _same_bits(S, S2) and _same_bits(S2, S2.T)


# ------------------------------------------------------------------------------------- (7) the model API

def test_model_prediction_full_cov():
    c = CASES["isomatern52"]
    X, y, Xt = c["X"], c["y"], c["Xt"]
    kern = dsm.IsoMatern52(float(c["loghyp"][0]), float(c["loghyp"][1]))
    gp = dsm.GaussianProcess(X, y, mean=dsm.ConstMean(float(c["mean"])), kernel=kern, logNoise=float(c["logNoise"]),
                             run_cholesky=True)
    mu0, var0 = dsm.prediction(gp, Xt)
    mu, S = dsm.prediction(gp, Xt, full_cov=True)
    mu1, var1 = dsm.prediction(gp, Xt, full_cov=False)
    assert _same_bits(mu0, mu) and _same_bits(mu0, mu1) and _same_bits(var0, var1)
    assert _same_bits(S, gp.model.ctx.predict_cov(0, Xt.shape[0], True))
    nt = Xt.shape[0]
    r, cc = packed_lower(nt)
    ref = np.zeros((nt, nt))
    ref[r, cc] = c["sigma"]
    ref[cc, r] = c["sigma"]
    noise = lib_noise(c["logNoise"])
    ref += noise * np.eye(nt)
    _check("model full_cov", S, ref, entry_tol(ref, c["kss"], noise))
    smp = dsm.posterior_sample(gp, Xt[:40], 5, seed=3)
    assert smp.shape == (5, 40) and np.all(np.isfinite(smp))
    assert _same_bits(smp, dsm.posterior_sample(gp, Xt[:40], 5, seed=3))
