"""CPU tests of the multi-target gradient path: the C ABI's declaration and export, the Julia ccall site, the float64 dense
restatement (tests/targets_grad_dense.py) against the 50-digit fixture (tests/golden/gp_targets_grad.npz), and the host side of
model.targets_objective / model.grad_targets / model.train(targets=...) over a stand-in context
(tests/targets_grad_context.py).  The default paths (train, grad_mll, grad_loo without targets) are pinned to the bits the
parent commit gave (tests/golden/targets_grad_parent.json, recorded by targets_grad_context.default_path_results)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_kernels as dk
import targets_grad_context as tgc
import targets_grad_dense as tgd
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel
from targets_grad_context import TargetsGradOracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = tgd.load_cases()


# ------------------------------------------------------------------------------------- the prototypes

def test_header_export_and_julia_prototype():
    assert hipabi.SIGNATURES["dsmgp_mll_columns_gradients"][1] == [hipabi._ctx, hipabi._dp, hipabi.C.c_int32, hipabi._dp, hipabi._dp]
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", header, flags=re.S))
    assert ("int dsmgp_mll_columns_gradients(dsmgp_ctx* ctx, double* grad_out , int32_t stride, const double* col_weight , "
            "double* seconds );") in flat
    for phrase in ("NOT counted by dsmgp_estimate_bytes", "The mask of dsmgp_set_gradient_leaves does not apply", "NULL = ones"):
        assert phrase in header, phrase
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "dsmgp_mll_columns_gradients" in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    # the name of the feature is an inline alias of the header, not a second symbol: a C99 caller compiles against it
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "dsmgp_targets_gradients" not in exported and "static inline int dsmgp_targets_gradients(" in header
    src = ('#include "dsmgp_hip.h"\nint f(dsmgp_ctx* c, double* g, const double* w) '
           '{ double s; return dsmgp_targets_gradients(c, g, 3, w, &s); }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    "-x", "c", "-"], input=src, text=True, check=True)
    julia = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    assert "ccall(sym(:dsmgp_mll_columns_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{Float64})" in julia
    assert "function targets_gradients(s::Session; col_weight" in julia
    assert "targets_gradients" in {t.strip() for t in re.search(r"(?m)^export ([^\n]*)", julia).group(1).split(",")}
    for cls in (hipabi.StreamingContext,):          # no targets path on the factor-and-discard context
        assert not hasattr(cls, "targets_gradients") and not hasattr(cls, "solve_targets")


# ------------------------------------------------------------------------------------- the fixture and the dense module

def test_fixture_covers_the_cases_the_feature_names():
    assert {int(c["kind"]) for c in CASES.values()} == set(range(11))
    assert {c["X"].shape[0] for c in CASES.values()} == {1, 2, 128, 130, 300}
    assert {c["Y"].shape[1] for c in CASES.values()} == {1, 3, 16, 17, 33}
    assert {c["X"].shape[1] for c in CASES.values()} == {1, 3}
    assert any(bool(c["weak"]) for c in CASES.values()) and any("grad_true" in c for c in CASES.values())
    for c in CASES.values():
        Q = c["Y"].shape[1]
        assert c["grad"].shape == (Q, c["hyp"].size) and np.array_equal(c["w"], tgd.signed_weights(Q))
        assert c["hyp"].size == dk.n_hyper(int(c["kind"]), c["X"].shape[1])
    assert os.path.getsize(os.path.join(GOLDEN, "gp_targets_grad.npz")) < (1 << 20)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_helper_against_50_digits(name):
    """Every column, the signed sum and the plain sum of the dense module within the tolerance of the 50-digit values."""
    c = CASES[name]
    kind, D = int(c["kind"]), c["X"].shape[1]
    tolk = dict(kind=kind, hyp=c["hyp"], weak=bool(c["weak"]), n=c["X"].shape[0], c_trKinv=float(c["c_trKinv"]))
    worst = 0.0
    for ard_true in ((False, True) if kind == 1 else (False,)):
        G, mll, cond = tgd.column_gradients(kind, c["hyp"], c["X"], c["Y"], c["mean"], ard_true=ard_true)
        assert 0.5 <= cond / float(c["cond"]) <= 2.0
        ref, wsum = c["grad"].copy(), c["wsum"].copy()
        if ard_true:
            ref[:, :D], wsum[:D] = c["grad_true"], c["wsum_true"]
        elif kind == 1:
            assert np.all(G[:, :D] == 0.0)
        Q = ref.shape[0]
        r = [np.max(np.abs(tgd.weighted(G, c["w"]) - wsum) / tgd.tolerance(ref, c["w"], c["cond"], **tolk))]
        for j in range(Q):
            e = np.zeros(Q)
            e[j] = 1.0
            r.append(np.max(np.abs(G[j] - ref[j]) / tgd.tolerance(ref, e, c["cond"], **tolk)))
        worst = max(worst, float(max(r)))
        assert np.max(np.abs(mll - c["mll"])) <= 64.0 * float(c["cond"]) * tgd.EPS * max(1.0, float(np.max(np.abs(c["mll"]))))
    print(f"\n{name}: worst err/tol {worst:.3g}")
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------------------------------------------- the tree recursions

def _problem(n, seed, D=2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, D))
    Y = np.stack([np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]), 5.0 + X[:, 0] - X[:, -1] ** 2, np.cos(4.0 * X[:, -1]) - 2.0], axis=1)
    return X, Y + 0.1 * rng.standard_normal(Y.shape)


def _model(family, X, y, kernel=None, seed=2):
    kw = dict(M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0) if kernel is None else kernel, logNoise=np.log(0.2),
              ctx=TargetsGradOracleContext(), seed=seed)
    if family == "dsmgp":
        return dsm.buildDSMGP(X, y, 2, 4, **kw)
    if family == "dsmgp_kernels":
        kw["kernel"] = [dsm.IsoSE(np.log(0.5), 0.0), dsm.IsoLinear(0.0)]
        return dsm.buildDSMGP(X, y, 2, 3, **kw)
    if family in ("poe", "gpoe"):
        return dsm.buildPoE(X, y, 4, meanFun=dsm.ConstMean(float(np.mean(y))), generalized=family == "gpoe", **kw)
    if family == "rbcm":
        return dsm.buildBCM(X, y, 4, robust=True, **kw)
    return dsm.GaussianProcess(X[:80], y[:80], kernel=kw["kernel"], logNoise=kw["logNoise"], ctx=TargetsGradOracleContext())


def _leaf_means(m):
    target = m.model if isinstance(m, dsm.GaussianProcess) else m
    return np.array([[lf_mean] for lf_mean in target.ctx.mean])


@pytest.mark.parametrize("family", ["dsmgp", "dsmgp_kernels", "poe", "gpoe", "rbcm", "gp"])
def test_grad_targets_with_the_models_own_y_equals_grad_mll(family):
    """Y = y[:, None] and the leaves' own means: targets_objective is mll(model) and grad_targets is grad_mll(model), to the
    rounding of the two routes (oracle leaf gradients against the dense module's); one device call."""
    X, Y = _problem(300, 33)
    m = _model(family, X, Y[:, 0])
    target = m.model if family == "gp" else m
    y = Y[:80, 0] if family == "gp" else Y[:, 0]
    dsm.fit(m)
    dsm.updategradients(m)
    ref = dsm.grad_mll(m)
    table = dsm.fit_targets(m, y[:, None], mean=_leaf_means(m))
    assert np.allclose(table[:, 0], target.leaf_mll, rtol=1e-11, atol=1e-10)
    assert abs(dsm.targets_objective(m) - dsm.mll(m)) <= 1e-9 * max(1.0, abs(dsm.mll(m)))
    calls = getattr(target.ctx, "targets_gradient_calls", 0)
    g = dsm.grad_targets(m)
    assert target.ctx.targets_gradient_calls == calls + 1
    assert g.shape == ref.shape
    assert np.max(np.abs(g - ref)) <= 1e-8 * max(1.0, float(np.max(np.abs(ref)))), (family, g, ref)


@pytest.mark.parametrize("family", ["dsmgp", "dsmgp_kernels", "rbcm", "gp"])
def test_grad_targets_is_additive_in_columns(family):
    X, Y = _problem(300, 34)
    m = _model(family, X, Y[:, 0])
    Yl = Y[:80] if family == "gp" else Y
    dsm.fit_targets(m, Yl)
    total, obj = dsm.grad_targets(m), dsm.targets_objective(m)
    parts, objs = [], []
    for j in range(3):
        dsm.fit_targets(m, Yl[:, j])
        parts.append(dsm.grad_targets(m))
        objs.append(dsm.targets_objective(m))
    assert abs(obj - sum(objs)) <= 1e-10 * max(1.0, abs(obj))
    scale = max(1.0, float(np.max(np.abs(parts))))
    assert np.max(np.abs(total - sum(parts))) <= 1e-10 * scale


def test_grad_targets_against_central_differences_of_the_tree_objective():
    """A DSMGP tree (sum over split nodes over GPs) with synthetic per-(leaf, column) tables: grad_targets is `∇mll!` column by
    column -- for one column exactly grad_mll on that column's table, and the weight table reproduces every leaf's weight."""
    X, Y = _problem(300, 35)
    m = _model("dsmgp", X, Y[:, 0])
    dsm.fit_targets(m, Y)
    W, visits = dmodel.targets_weight_table(m)
    assert W.shape == (m.L, 3) and sorted(v[0] for v in visits) == list(range(m.L))
    rows = np.random.default_rng(3).standard_normal((m.L, dsm.getparams(m).size))
    for q in range(3):
        m.leaf_mll, m.leaf_grad = m.targets_mll[:, q].copy(), rows
        one = np.zeros_like(W)
        one[:, q] = W[:, q]
        a = dmodel._scatter_leaf_rows(m, rows * one[:, q:q + 1], [(l, 1.0, o, s) for l, _, o, s in visits])
        b = dsm.grad_mll(m)
        assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, float(np.max(np.abs(b))))


@pytest.mark.parametrize("kernel", ["ardseproduct", "ardmatern52", "isomatern32", "ardrq"])
def test_single_gp_true_gradient_kinds_against_central_differences(kernel):
    """A single GaussianProcess with a kind whose gradient is the true derivative: grad_targets against central differences of
    targets_objective over the shared hyper-vector (the column means held fixed)."""
    X, Y = _problem(60, 36, D=2)
    k = {"ardseproduct": dsm.ArdSEProduct(np.log([0.5, 0.8]), 0.1), "ardmatern52": dsm.ArdMatern52(np.log([0.5, 0.8]), 0.1),
         "isomatern32": dsm.IsoMatern32(np.log(0.6), 0.0), "ardrq": dsm.ArdRQ(np.log([0.5, 0.8]), np.log(1.5), 0.1)}[kernel]
    gp = dsm.GaussianProcess(X, Y[:, 0], kernel=k, logNoise=np.log(0.2), ctx=TargetsGradOracleContext())
    means = dsm.targets_leaf_means(gp, Y)
    h0 = dsm.getparams(gp.model).copy()

    def objective(h):
        dsm.setparams(gp.model, h)
        dsm.update_cholesky(gp)
        dsm.fit_targets(gp, Y, mean=means)
        return dsm.targets_objective(gp)

    objective(h0)
    g = dsm.grad_targets(gp)
    assert g.size == h0.size
    for j in range(h0.size):
        hp, hm = h0.copy(), h0.copy()
        hp[j] += 1e-5
        hm[j] -= 1e-5
        fd = (objective(hp) - objective(hm)) / 2e-5
        assert abs(g[j] - fd) <= 2e-6 * max(1.0, abs(fd)), (kernel, j, g[j], fd)


# ------------------------------------------------------------------------------------- train

@pytest.mark.parametrize("family", ["dsmgp", "gp"])
def test_train_on_the_models_own_y_follows_train(family):
    """train(model, targets=y[:, None]) against train(model), step for step over a few iterations: the same history and the same
    hyper-vector to rounding.  The leaf means of fit_targets' default are the leaves' own (built without a mean function)."""
    X, Y = _problem(300, 37)
    y = Y[:80, 0] if family == "gp" else Y[:, 0]
    a, b = _model(family, X, Y[:, 0]), _model(family, X, Y[:, 0])
    _, ha = dsm.train(a, iterations=4, randinit=False)
    _, hb = dsm.train(b, iterations=4, randinit=False, targets=y[:, None])
    ta, tb = (m.model if family == "gp" else m for m in (a, b))
    assert ha.shape == hb.shape == (4,)
    assert np.max(np.abs(ha - hb)) <= 1e-9 * max(1.0, float(np.max(np.abs(ha)))), (ha, hb)
    assert np.max(np.abs(dsm.getparams(ta) - dsm.getparams(tb))) <= 1e-9
    assert tb.ctx.targets_gradient_calls == 4 and not hasattr(ta.ctx, "targets_gradient_calls")


def test_train_on_three_columns_raises_their_objective():
    X, Y = _problem(300, 38)
    m = _model("dsmgp", X, Y[:, 0])
    _, hist = dsm.train(m, iterations=6, randinit=False, targets=Y, optim=dsm.ADAM(eta=1e-2))
    assert hist.shape == (6,) and np.all(np.diff(hist) > 0.0)
    dsm.fit_targets(m, Y)
    assert dsm.targets_objective(m) > hist[0]


def test_refusals():
    X, Y = _problem(120, 5)
    m = _model("dsmgp", X, Y[:, 0])
    h0 = dsm.getparams(m).copy()
    with pytest.raises(ValueError):
        dsm.train(m, objective="loo", targets=Y, iterations=1)
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.grad_targets(m)                                 # before fit_targets
    assert e.value.code == hipabi.E_STATE
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.targets_objective(m)
    assert e.value.code == hipabi.E_STATE
    assert np.array_equal(dsm.getparams(m), h0)
    dsm.fit_targets(m, Y)
    dsm.fit(m)                                              # a later fit: the resident targets are stale
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.grad_targets(m)
    assert e.value.code == hipabi.E_STATE

    class Streaming:                    # a context without the targets path: refused before any side effect
        want_gradients = 0
        groups = None

    m._ctx = Streaming()
    with pytest.raises(NotImplementedError):
        dsm.train(m, targets=Y, iterations=1)
    assert np.array_equal(dsm.getparams(m), h0)


# ------------------------------------------------------------------------------------- the defaults

def test_default_paths_give_the_bits_of_the_parent_commit():
    """train, grad_mll and grad_loo without targets: the values recorded on the parent commit, to the bit."""
    ref = json.load(open(os.path.join(GOLDEN, "targets_grad_parent.json")))
    got = tgc.default_path_results()
    assert set(got) == set(ref)
    for k in sorted(ref):
        assert got[k] == ref[k], k
