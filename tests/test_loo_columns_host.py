"""CPU tests of the leave-one-out path of the target columns: the C ABI's declarations and exports, the Julia ccall sites, the
float64 dense restatement (tests/loo_columns_dense.py, both forms) against the 50-digit fixture
(tests/golden/gp_loo_columns.npz), and the host side of model.loo_targets / loo_targets_objective / grad_loo_targets /
train(targets=..., targets_objective="loo") over a stand-in context (tests/loo_columns_context.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_kernels as dk
import loo_columns_dense as lcd
from deepstructuredmixtures_amd import hipabi
from loo_columns_context import LooColumnsOracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = lcd.load_cases()
C = hipabi.C


# ------------------------------------------------------------------------------------- the prototypes

def test_header_exports_and_julia_prototypes():
    dp, ctx = hipabi._dp, hipabi._ctx
    assert hipabi.SIGNATURES["dsmgp_loo_columns"] == (C.c_int, [ctx, dp, C.c_int64, dp, dp, dp])
    assert hipabi.SIGNATURES["dsmgp_loo_columns_gradients"] == (C.c_int, [ctx, dp, C.c_int32, dp, dp, dp])
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert "int dsmgp_loo_columns(dsmgp_ctx* ctx, double* mu_out , int64_t ld, double* var_out , double* lpd_out , double* seconds );" in flat
    assert ("int dsmgp_loo_columns_gradients(dsmgp_ctx* ctx, double* grad_out , int32_t stride, const double* col_weight , "
            "double* lpd_out , double* seconds );") in flat
    out_of_scope = re.sub(r"\s+", " ", header[header.index("Out of scope"):header.index("int dsmgp_solve_targets(")])
    assert "LOO" not in out_of_scope.split("Gradients of")[0] and "input gradients" in out_of_scope and "streaming" in out_of_scope
    for phrase in ("NOT counted by dsmgp_estimate_bytes", "a non-finite or negative weight", "NULL = ones"):
        assert phrase in header, phrase
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    new = {"dsmgp_loo_columns", "dsmgp_loo_columns_gradients"}
    assert new <= exported and not any("target" in s.lower() for s in new)
    assert {s for s in exported if "loo_columns" in s and not s.startswith("_Z")} == new     # (_Z...: the kernels' host stubs)
    julia = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    flatj = re.sub(r"\s+", " ", julia)
    assert ("ccall(sym(:dsmgp_loo_columns), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ref{Float64})"
            in flatj)
    assert ("ccall(sym(:dsmgp_loo_columns_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}, "
            "Ref{Float64})") in flatj
    assert "function loo_targets(s::Session)" in julia and "function loo_targets_gradients(s::Session; col_weight" in julia
    assert {"loo_targets", "loo_targets_gradients"} <= {t.strip() for t in re.search(r"(?m)^export ([^\n]*)", julia).group(1).split(",")}
    assert hasattr(hipabi.Context, "loo_targets") and hasattr(hipabi.Context, "loo_targets_gradients")
    for cls in (c for c in vars(hipabi).values() if isinstance(c, type)):
        assert hasattr(cls, "loo_targets") == hasattr(cls, "solve_targets") == hasattr(cls, "loo_targets_gradients"), cls
    assert not hasattr(hipabi.StreamingContext, "loo_targets") and not hasattr(hipabi.StreamingContext, "loo_targets_gradients")


# ------------------------------------------------------------------------------------- the fixture and the dense module

def test_fixture_covers_the_cases_the_feature_names():
    assert {c["kind"] for c in CASES.values()} == set(range(11))
    assert max(c["X"].shape[0] for c in CASES.values()) <= 40
    assert {c["Y"].shape[1] for c in CASES.values()} == {1, 3}
    assert any(c["weak"] and c["kind"] == 2 for c in CASES.values())
    assert any(np.any(c["w"] == 0.0) for c in CASES.values()) and all(np.all(c["w"] >= 0.0) for c in CASES.values())
    for c in CASES.values():
        n, Q = c["Y"].shape
        assert c["mu"].shape == (n, Q) and c["var"].shape == (n,) and c["lpd"].shape == (Q,)
        assert c["grad"].shape == (Q, c["hyp"].size) and c["wsum"].shape == (c["hyp"].size,) and c["cond"] >= 1.0
        assert np.array_equal(c["w"], lcd.weights(Q))
    assert os.path.getsize(os.path.join(GOLDEN, "gp_loo_columns.npz")) < (1 << 19)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_module_against_50_digits(name):
    """The moments, every column's gradient by the literal form, and the weighted sum by both forms, within the tolerances of
    the 50-digit values."""
    c = CASES[name]
    kind, hyp, X, Y, mean, w = c["kind"], c["hyp"], c["X"], c["Y"], c["mean"], c["w"]
    Q = Y.shape[1]
    mu, var, lpd = lcd.moments(kind, hyp, X, Y, mean)
    r = []
    for q in range(Q):
        tm, tv, _, ts = lcd.moment_tolerances(c, q)
        r += [np.max(np.abs(mu[:, q] - c["mu"][:, q]) / tm), np.max(np.abs(var - c["var"]) / tv), abs(lpd[q] - c["lpd"][q]) / ts]
    G = lcd.column_gradients_literal(kind, hyp, X, Y, mean)
    for q in range(Q):
        e = np.zeros(Q)
        e[q] = 1.0
        r.append(np.max(np.abs(G[q] - c["grad"][q]) / lcd.gradient_tolerance(c, c["grad"], e)))
        r.append(np.max(np.abs(lcd.weighted_gradient(kind, hyp, X, Y, mean, e) - c["grad"][q]) / lcd.gradient_tolerance(c, c["grad"], e)))
    tol = lcd.gradient_tolerance(c, c["grad"], w)
    r.append(np.max(np.abs(lcd.weighted(G, w) - c["wsum"]) / tol))
    r.append(np.max(np.abs(lcd.weighted_gradient(kind, hyp, X, Y, mean, w) - c["wsum"]) / tol))
    print(f"\n{name}: worst err/tol {max(r):.3g}")
    assert max(r) <= 1.0, (name, r)


def test_dense_moments_against_brute_force_refits():
    """n = 9, Q = 3: the moments equal a GP refitted without the row, column by column (loo_dense.loo_brute)."""
    import loo_dense as ld
    rng = np.random.default_rng(4)
    X = rng.uniform(size=(9, 2))
    Y = np.stack([np.sin(3.0 * X[:, 0]), X[:, 1] + 2.0, rng.standard_normal(9)], axis=1)
    mean = np.array([0.1, 2.4, 0.0])
    hyp = np.array([np.log(0.5), 0.1, np.log(0.2)])
    mu, var, _ = lcd.moments(0, hyp, X, Y, mean)
    K = dk.d_hyper(0, hyp[:-1], X)[0]
    for q in range(3):
        mb, vb = ld.loo_brute(K, np.exp(2.0 * hyp[-1]), Y[:, q], mean[q])
        assert np.allclose(mu[:, q], mb, rtol=1e-9, atol=1e-10) and np.allclose(var, vb + ld.JITTER, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------- the tree recursions

def _problem(n, seed, D=2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, D))
    Y = np.stack([np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]), 5.0 + X[:, 0] - X[:, -1] ** 2, np.cos(4.0 * X[:, -1]) - 2.0], axis=1)
    return X, Y + 0.1 * rng.standard_normal(Y.shape)


def _model(family, X, y, kernel=None, seed=2):
    kw = dict(M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0) if kernel is None else kernel, logNoise=np.log(0.2),
              ctx=LooColumnsOracleContext(), seed=seed)
    if family == "dsmgp":
        return dsm.buildDSMGP(X, y, 2, 4, **kw)
    if family == "dsmgp_kernels":
        kw["kernel"] = [dsm.IsoSE(np.log(0.5), 0.0), dsm.IsoLinear(0.0)]
        return dsm.buildDSMGP(X, y, 2, 3, **kw)
    if family == "poe":
        return dsm.buildPoE(X, y, 4, meanFun=dsm.ConstMean(float(np.mean(y))), **kw)
    return dsm.GaussianProcess(X[:60], y[:60], kernel=kw["kernel"], logNoise=kw["logNoise"], ctx=LooColumnsOracleContext())


@pytest.mark.parametrize("family", ["dsmgp", "dsmgp_kernels", "poe", "gp"])
def test_grad_loo_targets_against_central_differences_of_the_objective(family):
    """loo_targets_objective over the shared hyper-vector (the column means held fixed): grad_loo_targets is its true gradient,
    from ONE device call."""
    X, Y = _problem(120, 41)
    m = _model(family, X, Y[:, 0])
    target = m.model if family == "gp" else m
    Yl = Y[:60] if family == "gp" else Y
    dsm.fit(m)
    means = dsm.targets_leaf_means(m, Yl)
    h0 = dsm.getparams(target).copy()

    def objective(h):
        dsm.setparams(target, h)
        dsm.update_cholesky(m) if family == "gp" else dsm.fit(m)
        dsm.fit_targets(m, Yl, mean=means)
        return dsm.loo_targets_objective(m)

    obj = objective(h0)
    res = dsm.loo_targets(m)
    assert res["lpd"].shape == (target.L, 3) and all(res["mu"][l].shape == (len(target.leaves[l].obs), 3) for l in range(target.L))
    assert all(res["var"][l].shape == (len(target.leaves[l].obs),) for l in range(target.L))
    assert abs(dsm.loo_targets_objective(m, lpd=res["lpd"]) - obj) <= 1e-12 * max(1.0, abs(obj))
    calls = getattr(target.ctx, "loo_targets_gradient_calls", 0)
    g = dsm.grad_loo_targets(m)
    assert target.ctx.loo_targets_gradient_calls == calls + 1 and g.size == h0.size
    for j in range(h0.size):
        hp, hm = h0.copy(), h0.copy()
        hp[j] += 1e-5
        hm[j] -= 1e-5
        fd = (objective(hp) - objective(hm)) / 2e-5
        assert abs(g[j] - fd) <= 2e-6 * max(1.0, abs(fd)), (family, j, g[j], fd)


@pytest.mark.parametrize("family", ["dsmgp", "dsmgp_kernels", "poe", "gp"])
def test_one_column_with_the_models_own_y_reduces_to_loo_objective_and_grad_loo(family):
    X, Y = _problem(120, 42)
    m = _model(family, X, Y[:, 0])
    target = m.model if family == "gp" else m
    y = Y[:60, 0] if family == "gp" else Y[:, 0]
    dsm.fit(m)
    lpd = np.array([lcd.moments(target.ctx.hyper[target.ctx.kid[i]][0], np.asarray(target.ctx.hyper[target.ctx.kid[i]][1]),
                                target.ctx.X[target.ctx.obs[i]], y[target.ctx.obs[i]], [target.ctx.mean[i]])[2][0]
                    for i in range(target.L)])
    ref_obj = dsm.loo_objective(m, lpd=lpd)
    dsm.fit_targets(m, y[:, None], mean=np.array([[v] for v in target.ctx.mean]))
    assert abs(dsm.loo_targets_objective(m) - ref_obj) <= 1e-12 * max(1.0, abs(ref_obj))
    g = dsm.grad_loo_targets(m)
    target.leaf_lpd = lpd                       # grad_loo on the same table and the same per-leaf rows
    target.leaf_grad = target.ctx.loo_targets_gradients(g.size if family == "gp" else max(lf.kernel.nparams() + 1 for lf in target.leaves))[0]
    ref = dsm.grad_loo(m)
    assert g.shape == ref.shape and np.max(np.abs(g - ref)) <= 1e-12 * max(1.0, float(np.max(np.abs(ref))))


# ------------------------------------------------------------------------------------- train

def test_train_on_the_loo_density_of_three_columns_raises_it():
    X, Y = _problem(150, 43)
    m = _model("dsmgp", X, Y[:, 0])
    _, hist = dsm.train(m, iterations=5, randinit=False, targets=Y, targets_objective="loo", optim=dsm.ADAM(eta=1e-2))
    assert hist.shape == (5,) and np.all(np.diff(hist) > 0.0)
    assert m.ctx.loo_targets_gradient_calls == 5 and not hasattr(m.ctx, "targets_gradient_calls")
    dsm.fit_targets(m, Y)
    assert dsm.loo_targets_objective(m) > hist[0]
    a, b = _model("dsmgp", X, Y[:, 0]), _model("dsmgp", X, Y[:, 0])
    _, ha = dsm.train(a, iterations=3, randinit=False, targets=Y)
    _, hb = dsm.train(b, iterations=3, randinit=False, targets=Y, targets_objective="mll")     # the default: nothing changes
    assert np.array_equal(ha, hb) and np.array_equal(dsm.getparams(a), dsm.getparams(b))
    gp = _model("gp", X, Y[:, 0])
    _, hg = dsm.train(gp, iterations=3, randinit=False, targets=Y[:60], targets_objective="loo")
    assert hg.shape == (3,) and np.all(np.isfinite(hg))


def test_refusals():
    X, Y = _problem(120, 5)
    m = _model("dsmgp", X, Y[:, 0])
    h0 = dsm.getparams(m).copy()
    with pytest.raises(ValueError):
        dsm.train(m, objective="loo", targets=Y, iterations=1)
    with pytest.raises(ValueError):
        dsm.train(m, objective="loo", targets=Y, targets_objective="loo", iterations=1)
    for bad in ("elbo", None, "LOO"):
        with pytest.raises(ValueError):
            dsm.train(m, targets=Y, targets_objective=bad, iterations=1)
    for fn in (dsm.grad_loo_targets, dsm.loo_targets, dsm.loo_targets_objective):
        with pytest.raises(hipabi.DsmgpError) as e:
            fn(m)                                           # before fit_targets
        assert e.value.code == hipabi.E_STATE
    assert np.array_equal(dsm.getparams(m), h0)
    dsm.fit_targets(m, Y)
    dsm.loo_targets(m)
    dsm.fit(m)                                              # a later fit: the resident targets are stale
    for fn in (dsm.grad_loo_targets, dsm.loo_targets):
        with pytest.raises(hipabi.DsmgpError) as e:
            fn(m)
        assert e.value.code == hipabi.E_STATE
    dsm.fit_targets(m, Y)
    with pytest.raises(hipabi.DsmgpError) as e:
        m.ctx.loo_targets_gradients(3, -np.ones((m.L, 3)))
    assert e.value.code == hipabi.E_ARG

    class Streaming:                    # a context without the targets path: refused before any side effect
        want_gradients = 0
        groups = None

    m._ctx = Streaming()
    for fn in (dsm.loo_targets, dsm.grad_loo_targets):
        with pytest.raises(NotImplementedError):
            fn(m)
    with pytest.raises(NotImplementedError):
        dsm.train(m, targets=Y, targets_objective="loo", iterations=1)
    assert np.array_equal(dsm.getparams(m), h0)
