"""CPU tests of the several-target-columns path: the C ABI's declarations and exports, the Julia ccall sites, the float64 dense
restatement (tests/targets_dense.py) against the 50-digit fixture (tests/golden/gp_targets.npz), and the host side of
model.fit_targets / model.predict_targets -- default means and the column-by-column aggregation against the oracle's rules --
over a stand-in context (tests/targets_context.py)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_gp
import dense_kernels as dk
import targets_dense as td
from deepstructuredmixtures_amd import hipabi
from oracle import gp as ogp
from oracle import spn as ospn
from targets_context import TargetsOracleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = {"dsmgp_solve_targets": ("int", ["dsmgp_ctx*", "double*", "int64_t", "int32_t", "int64_t", "double*", "double*", "double*"]),
       "dsmgp_predict_targets": ("int", ["dsmgp_ctx*", "double*", "int64_t", "double*"]),
       "dsmgp_targets_fetch": ("int", ["dsmgp_ctx*", "int32_t", "double*"])}
CASES = td.load_cases()


def _header_prototypes():
    """name -> (return type, [argument types]) of every function include/dsmgp_hip.h declares, comments and `const` dropped."""
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b((?:const\s+)?(?:int64_t|int|char|void|double)\s*\**)\s*(dsmgp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        def norm(t):
            mm = re.match(r"\s*([A-Za-z_]\w*)\s*((?:\*\s*)*)", re.sub(r"\bconst\b", " ", t))
            return mm.group(1) + "*" * mm.group(2).count("*")
        args = m.group(3)
        protos[m.group(2)] = (norm(m.group(1)), [norm(a) for a in args.split(",")] if args.strip() not in ("", "void") else [])
    return protos


def test_header_declares_and_library_exports_the_three_functions():
    protos = _header_prototypes()
    for name, sig in NEW.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert name in hipabi.SIGNATURES and len(hipabi.SIGNATURES[name][1]) == len(sig[1])
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
    # exactly what is declared is exported: nothing of the new path beside the three
    assert {s for s in exported if "target" in s.lower() and not s.startswith("_Z")} == set(NEW)        # (_Z...: the kernels' host stubs)
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    for phrase in ("var_out for every column", "NOT counted by dsmgp_estimate_bytes", "Out of scope"):
        assert phrase in header, phrase


_JL_TO_C = {"Int32": "int32_t", "Int64": "int64_t", "Cint": "int", "Ptr{Float64}": "double*", "Ref{Float64}": "double*",
            "Ptr{Cvoid}": "dsmgp_ctx*"}


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


def test_julia_ccall_sites_match_the_header():
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    seen = set()
    for m in re.finditer(r"ccall\(", src):
        parts = _ccall_parts(src, m.end())
        name = re.match(r"sym\(:(\w+)\)$", parts[0]).group(1)
        if name not in NEW:
            continue
        seen.add(name)
        ret, args = NEW[name]
        types = [t.strip() for t in parts[2][1:-1].split(",") if t.strip()]
        assert _JL_TO_C[parts[1]] == ret
        assert [_JL_TO_C[t] for t in types] == args, (name, types)
        assert len(parts) - 3 == len(args), (name, parts[3:])
    assert seen == set(NEW)
    for fn in ("solve_targets(s::Session, Y::AbstractMatrix; mean", "predict_targets(s::Session)", "targets_fetch(s::Session, leaf::Integer)"):
        assert "function " + fn in src, fn
    export = re.search(r"(?m)^export ([^\n]*)", src).group(1)
    assert {"solve_targets", "predict_targets", "targets_fetch"} <= {t.strip() for t in export.split(",")}


def test_fixture_covers_the_cases_the_feature_names():
    shapes = {(c["kind"], c["X"].shape[0]) for c in CASES.values()}
    assert {(0, 37), (8, 129), (2, 130)} <= shapes
    assert all(c["Y"].shape[1] == 3 and c["X"].shape[1] in (2, 3) and 1 <= c["Xt"].shape[0] <= 8 for c in CASES.values())
    assert any(math.exp(2.0 * c["logNoise"]) <= 1e-8 * (1 + 1e-9) for c in CASES.values())        # noise at the jitter floor
    assert os.path.getsize(os.path.join(GOLDEN, "gp_targets.npz")) <= os.path.getsize(os.path.join(GOLDEN, "gp_loo.npz"))


def _kernel_matrix(c, A, B):
    """The kernel of a fixture case in float64 (kinds 0, 2 through the oracle, ArdMatern52 from tests/dense_kernels.py)."""
    h = c["loghyp"]
    if c["kind"] in (0, 2):
        return ogp.kernelmatrix(ogp.make_kernel(c["kind"], h), A, B, True)
    return dk.value(c["kind"], h, A, B)


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_helper_against_50_digits(name):
    c = CASES[name]
    F = dense_gp.factor(_kernel_matrix(c, c["X"], c["X"]), math.exp(2.0 * c["logNoise"]))
    cond = td.factor_cond(F)
    assert 0.5 <= cond / c["cond"] <= 2.0
    Z, mll, mu = td.reference(F, c["Y"], c["mean"], _kernel_matrix(c, c["Xt"], c["X"]))
    r = [np.max(np.abs(Z - c["Z"]) / td.z_tol(c["Z"], cond)), np.max(np.abs(mll - c["mll"]) / td.mll_tol(c["Z"], F, cond)),
         np.max(np.abs(mu - c["mu"]) / td.mu_tol(c["mu"], c["Y"]))]
    print(f"\n{name}: cond {cond:.3g}, dense err/tol Z {r[0]:.3g} mll {r[1]:.3g} mu {r[2]:.3g}")
    assert max(r) <= 1.0, (name, r)
    # column j alone is column j of the table (to rounding: the BLAS solves one and three right-hand sides differently)
    Z1, mll1, _ = td.reference(F, c["Y"][:, 1], c["mean"][1])
    assert np.all(np.abs(Z1[:, 0] - Z[:, 1]) <= td.z_tol(c["Z"], cond)[:, 1]) and abs(mll1[0] - mll[1]) <= td.mll_tol(c["Z"], F, cond)[1]


def _problem(n, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    Y = np.stack([np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]), 5.0 + X[:, 0] - X[:, 1] ** 2, np.cos(4.0 * X[:, 1]) - 2.0], axis=1)
    Y += 0.1 * rng.standard_normal(Y.shape)
    xt = rng.uniform(size=(20, 2)) * 0.98 + 0.01
    return X, Y, xt


def _column_gps(m, X, Y, means, j):
    gps = []
    for l, lf in enumerate(ospn.get_leaves(m.root)):
        k = ogp.make_kernel(lf.kernel.kind, lf.kernel.loghyp())
        gps.append(ogp.GaussianProcess(X[lf.obs], Y[lf.obs, j], means[l, j], k, lf.logNoise, True).update_cholesky())
    return gps


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gpoe", "rbcm", "gp"])
def test_host_aggregation_column_by_column_against_the_oracle(family):
    """predict_targets aggregates the per-column leaf moments with the model's own rule: column j equals the oracle's aggregation
    over oracle leaves that were given y_j and the same means; the default means are mean(Y[obs], axis=0) per leaf."""
    X, Y, xt = _problem(300, 33)
    kw = dict(M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.2), ctx=TargetsOracleContext(), seed=2)
    if family == "dsmgp":
        m, ofun = dsm.buildDSMGP(X, Y[:, 0], 2, 4, **kw), ospn.predict
        dsm.update(m)
    elif family in ("poe", "gpoe"):
        m = dsm.buildPoE(X, Y[:, 0], 4, meanFun=dsm.ConstMean(0.2), generalized=family == "gpoe", **kw)
        ofun = ospn.predict_gpoe if family == "gpoe" else ospn.predict_poe
    elif family == "rbcm":
        m, ofun = dsm.buildBCM(X, Y[:, 0], 4, **kw), ospn.predict_rbcm
    else:
        X, Y = X[:80], Y[:80]
        m = dsm.GaussianProcess(X, Y[:, 0], kernel=kw["kernel"], logNoise=kw["logNoise"], ctx=TargetsOracleContext())
    target = m.model if family == "gp" else m
    means = dsm.targets_leaf_means(m, Y)
    assert means.shape == (target.L, 3)
    for l, lf in enumerate(target.leaves):
        assert np.array_equal(means[l], np.mean(Y[lf.obs], axis=0))
    table = dsm.fit_targets(m, Y)                   # fits first where the model has no fit (the GaussianProcess)
    assert table.shape == (target.L, 3) and np.all(np.isfinite(target.leaf_mll))
    mu, var = dsm.predict_targets(m, xt)
    assert mu.shape == (20, 3) and var.shape == (20, 3)
    for j in range(3):
        gps = _column_gps(target, X, Y, means, j)
        assert np.allclose(table[:, j], [g.mll() for g in gps], rtol=1e-10, atol=1e-9)
        if family == "gp":
            mo, vo = gps[0].prediction(xt)
            vo = np.where(vo <= 0, 1e-8, vo)
        else:
            mo, vo = ofun(m.root, gps, xt)
        assert np.allclose(mu[:, j], mo, rtol=1e-9, atol=1e-10), (family, j)
        assert np.allclose(var[:, j], vo, rtol=1e-8, atol=1e-10), (family, j)
    if family in ("poe", "gpoe", "rbcm", "gp"):     # the product-of-experts variances do not depend on the column
        assert np.array_equal(var[:, 0], var[:, 1]) and np.array_equal(var[:, 0], var[:, 2])
    else:                                           # the mixture's does, through sum W mu^2 - mu^2
        assert not np.array_equal(var[:, 0], var[:, 1])
    # explicit means, and a vector as one column
    t1 = dsm.fit_targets(m, Y[:, 1], mean=means[:, 1:2])
    assert np.allclose(t1[:, 0], table[:, 1], rtol=1e-12, atol=1e-12)


def test_refusals_without_a_device():
    X, Y, xt = _problem(120, 5)
    m = dsm.buildPoE(X, Y[:, 0], 2, M=60, meanFun=dsm.ConstMean(0.0), kernel=dsm.IsoSE(0.0, 0.0), ctx=TargetsOracleContext(), seed=1)
    with pytest.raises(ValueError):
        dsm.fit_targets(m, Y[:-1])
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.predict_targets(m, xt)                  # before fit_targets
    assert e.value.code == hipabi.E_STATE
    dsm.fit_targets(m, Y)
    mu, var = dsm.predict_targets(m, np.zeros((0, 2)))
    assert mu.shape == (0, 3) and var.shape == (0, 3)
