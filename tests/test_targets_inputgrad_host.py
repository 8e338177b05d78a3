"""CPU tests of the input gradients of the multi-target predictive means: the C ABI's declaration and export, the SIGNATURES entry
and the Julia ccall site of dsmgp_predict_columns_gradients, and the host side of model.predict_targets_gradients over a stand-in
context (tests/targets_inputgrad_context.py): column j against predict_gradients of a model built on Y[:, j], against central
differences of predict_targets, and the refusals.  No device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi
from targets_inputgrad_context import TargetsInputGradOracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dsmgp_predict_columns_gradients"
SIG = ("int", ["dsmgp_ctx*", "double*", "int64_t", "double*"])
_JL_TO_C = {"Int32": "int32_t", "Int64": "int64_t", "Cint": "int", "Ptr{Float64}": "double*", "Ref{Float64}": "double*",
            "Ptr{Cvoid}": "dsmgp_ctx*"}
_C_TO_CT = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "dsmgp_ctx*": hipabi._ctx, "double*": hipabi._dp}


def _header_prototypes():
    """name -> (return type, [argument types]) of every function include/dsmgp_hip.h declares, comments and `const` dropped
    (the helper of tests/test_targets_host.py)."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b((?:const\s+)?(?:int64_t|int|char|void|double)\s*\**)\s*(dsmgp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        def norm(t):
            mm = re.match(r"\s*([A-Za-z_]\w*)\s*((?:\*\s*)*)", re.sub(r"\bconst\b", " ", t))
            return mm.group(1) + "*" * mm.group(2).count("*")
        args = m.group(3)
        protos[m.group(2)] = (norm(m.group(1)), [norm(a) for a in args.split(",")] if args.strip() not in ("", "void") else [])
    return protos


def _ccall_parts(src, at):
    """The top-level comma-separated parts of the ccall( that opens at `at`."""
    depth, j = 1, at
    while depth:
        depth += src[j] in "([{"
        depth -= src[j] in ")]}"
        j += 1
    parts, cur, depth = [], "", 0
    for ch in src[at:j - 1]:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return parts + [cur.strip()]


def test_header_signatures_and_julia_agree():
    assert _header_prototypes().get(NAME) == SIG
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    assert "static inline int dsmgp_predict_targets_gradients(" in header
    for phrase in ("Out of scope", "var_out for every column", "NOT counted by dsmgp_estimate_bytes",
                   "dsmgp_predict_gradients' dvar_out for every column"):
        assert phrase in header, phrase
    out_of_scope = re.sub(r"\s+", " ", header[header.index("Out of scope"):header.index("int dsmgp_solve_targets(")])
    assert NAME in out_of_scope and "input gradients for the extra columns" not in out_of_scope
    ret, args = hipabi.SIGNATURES[NAME]
    assert ret is _C_TO_CT[SIG[0]] and list(args) == [_C_TO_CT[a] for a in SIG[1]]
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    sites = 0
    for m in re.finditer(r"ccall\(", src):
        parts = _ccall_parts(src, m.end())
        if re.match(r"sym\(:(\w+)\)$", parts[0]).group(1) != NAME:
            continue
        sites += 1
        types = [t.strip() for t in parts[2][1:-1].split(",") if t.strip()]
        assert _JL_TO_C[parts[1]] == SIG[0] and [_JL_TO_C[t] for t in types] == SIG[1], types
        assert len(parts) - 3 == len(SIG[1]), parts[3:]
    assert sites == 1
    assert "function predict_targets_gradients(s::Session)" in src
    export = re.search(r"(?m)^export ([^\n]*)", src).group(1)
    assert "predict_targets_gradients" in {t.strip() for t in export.split(",")}


def test_library_exports_the_symbol():
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert NAME in exported and "target" not in NAME.lower()


def _problem(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    Y = np.stack([np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]), 5.0 + X[:, 0] - X[:, 1] ** 2, np.cos(4.0 * X[:, 1]) - 2.0], axis=1)
    Y += 0.1 * rng.standard_normal(Y.shape)
    xt = rng.uniform(size=(12, 2)) * 0.98 + 0.01
    return X, Y, xt


LOGL, LOGNOISE = float(np.log(0.5)), float(np.log(0.2))


def _sum_nodes(node):
    out = [node] if node.kind == "sum" else []
    for c in getattr(node, "children", []):
        out += _sum_nodes(c)
    return out


def _build(family, X, y):
    """The same tree for every y (the splits read X and the seed only); the sum nodes get fixed, normalised, non-uniform weights."""
    kw = dict(M=30, kernel=dsm.IsoSE(LOGL, 0.0), logNoise=LOGNOISE, ctx=TargetsInputGradOracleContext(), seed=2)
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 2, 4, **kw)
        for s in _sum_nodes(m.root):
            w = 1.0 + np.arange(len(s.children), dtype=np.float64)
            s.logweights = np.log(w / np.sum(w))
        assert m.tindex.weights_normalised()
    elif family == "gpoe":
        m = dsm.buildPoE(X, y, 4, meanFun=dsm.ConstMean(0.2), generalized=True, **kw)
    elif family == "rbcm":
        m = dsm.buildBCM(X, y, 4, **kw)
    else:
        m = dsm.GaussianProcess(X, y, kernel=kw["kernel"], logNoise=kw["logNoise"], ctx=TargetsInputGradOracleContext())
    return m


@pytest.mark.parametrize("family", ["dsmgp", "gpoe", "rbcm", "gp"])
def test_columns_against_single_target_models_and_central_differences(family):
    """Column j of predict_targets_gradients equals predict_gradients of a model built on Y[:, j] with the same tree and weights
    (to rounding: the leaf means are the same numbers summed in another order), and the whole result agrees with central
    differences of predict_targets: step h = 1e-5 l and the bound 1e-6 (|f'| + scale / l) of
    test_predgrad_host.test_dense_helper_against_central_differences, scale = max(1, max|y_j|) for the means and
    max(1, k** + noise) for the variances."""
    X, Y, xt = _problem(300 if family != "gp" else 80, 33)
    m = _build(family, X, Y[:, 0])
    target = m.model if family == "gp" else m
    means = np.full((target.L, 3), 0.2) if family == "gpoe" else None
    dsm.fit_targets(m, Y, mean=means)
    mu, var, dmu, dvar = dsm.predict_targets_gradients(m, xt)
    n_t, D, Q = xt.shape[0], 2, 3
    assert mu.shape == (n_t, Q) and var.shape == (n_t, Q) and dmu.shape == (n_t, Q, D) and dvar.shape == (n_t, Q, D)
    mu0, var0 = dsm.predict_targets(m, xt)
    assert np.array_equal(mu, mu0) and np.array_equal(var, var0)
    for j in range(Q):
        mj = _build(family, X, Y[:, j])
        if family != "gp":
            dsm.fit(mj)
        else:
            dsm.update_cholesky(mj)
        a = dsm.predict_gradients(mj, xt)
        for got, ref in zip((mu[:, j], var[:, j], dmu[:, j], dvar[:, j]), a):
            assert np.allclose(got, ref, rtol=1e-9, atol=1e-10), (family, j)
    if family == "dsmgp":       # the mixture's variance depends on the column through the means
        assert not np.array_equal(dvar[:, 0], dvar[:, 1])
    else:
        assert np.array_equal(dvar[:, 0], dvar[:, 1]) and np.array_equal(dvar[:, 0], dvar[:, 2])
    ld = float(np.exp(LOGL))
    h = 1e-5 * ld
    vscale = max(1.0, 1.0 + float(np.exp(2 * LOGNOISE)))
    for d in range(D):
        E = np.zeros_like(xt)
        E[:, d] = h
        (mp_, vp), (mm, vm) = dsm.predict_targets(m, xt + E), dsm.predict_targets(m, xt - E)
        fm, fv = (mp_ - mm) / (2 * h), (vp - vm) / (2 * h)
        for j in range(Q):
            yscale = max(1.0, float(np.max(np.abs(Y[:, j]))))
            bm = 1e-6 * (np.abs(dmu[:, j, d]) + yscale / ld)
            bv = 1e-6 * (np.abs(dvar[:, j, d]) + vscale / ld)
            assert np.all(np.abs(fm[:, j] - dmu[:, j, d]) <= bm), (family, j, d, np.max(np.abs(fm[:, j] - dmu[:, j, d]) / bm))
            assert np.all(np.abs(fv[:, j] - dvar[:, j, d]) <= bv), (family, j, d, np.max(np.abs(fv[:, j] - dvar[:, j, d]) / bv))


def test_refusals():
    from targets_context import TargetsOracleContext
    X, Y, xt = _problem(200, 5)
    m = _build("dsmgp", X, Y[:, 0])
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.predict_targets_gradients(m, xt)                # before fit_targets
    assert e.value.code == hipabi.E_STATE
    dsm.fit_targets(m, Y)
    out = dsm.predict_targets_gradients(m, np.zeros((0, 2)))
    assert [o.shape for o in out] == [(0, 3), (0, 3), (0, 3, 2), (0, 3, 2)]
    s = _sum_nodes(m.root)[0]
    s.logweights = s.logweights + 0.3                       # weights that no longer add up to one
    with pytest.raises(ValueError, match="not normalised"):
        dsm.predict_targets_gradients(m, xt)
    m2 = dsm.buildDSMGP(X, Y[:, 0], 2, 4, M=30, kernel=dsm.IsoSE(LOGL, 0.0), logNoise=LOGNOISE, ctx=TargetsOracleContext(), seed=2)
    dsm.fit_targets(m2, Y)
    with pytest.raises(NotImplementedError, match="has no predict_targets_gradients"):      # a context without the device call
        dsm.predict_targets_gradients(m2, xt)
    world = m2.shard.world
    m2.shard.world = 2
    try:
        with pytest.raises(NotImplementedError, match="several ranks"):
            dsm.predict_targets_gradients(m2, xt)
    finally:
        m2.shard.world = world
    sc = hipabi.StreamingContext.__new__(hipabi.StreamingContext)
    with pytest.raises(hipabi.DsmgpError) as e:
        sc.predict_targets_gradients()
    assert e.value.code == hipabi.E_STATE
