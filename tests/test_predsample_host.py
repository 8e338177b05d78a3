"""CPU tests of the host side of the joint draws: model.posterior_sample(device=True), model.leaf_samples, model.mixture_sample
and the refusals on a NumPy test double (predsample_dense.OracleSampleContext); the selection law of mixture_sample; the new row
of csrc/ctx_state.hpp; the bindings' tables."""
import json
import os
import re
import subprocess
import types

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi, datagen, model as dmodel
from deepstructuredmixtures_amd.model import EPS
from deepstructuredmixtures_amd.tree import GPNode, GPSumNode
from predsample_dense import OracleSampleContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _problem(N=160, D=2, seed=31, nt=30):
    X = datagen.uniform(seed, 0, N * D).reshape((N, D), order="F")
    y = np.sin(5 * X[:, 0]) + 0.5 * X[:, -1] + 0.1 * datagen.normal(seed + 1, 0, N)
    Xt = datagen.uniform(seed + 2, 0, nt * D).reshape((nt, D), order="F")
    return X, y, Xt


def _gp(X, y):
    return dsm.GaussianProcess(X, y, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), ctx=OracleSampleContext(),
                               run_cholesky=True)


def _tree_model(X, y):
    return dsm.buildDSMGP(X, y, 2, 3, M=40, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), seed=5,
                          ctx=OracleSampleContext())


def test_posterior_sample_default_returns_the_bits_it_returned_before():
    """Without `device` the call is the parent commit's: predict_cov, + EPS without noise, np.linalg.cholesky, the product --
    operation for operation, and predict_sample is never called."""
    X, y, Xt = _problem()
    gp = _gp(X, y)
    nt, ns = Xt.shape[0], 7
    for with_noise in (False, True):
        s = dsm.posterior_sample(gp, Xt, ns, seed=11, with_noise=with_noise)
        mu, _ = dsm.prediction(gp, Xt)
        S = gp.model.ctx.predict_cov(0, nt, with_noise)
        if not with_noise:
            S[np.arange(nt), np.arange(nt)] += EPS
        eps = datagen.normal(11, 0, nt * ns).reshape((nt, ns), order="F")
        assert np.array_equal(s, (mu[:, None] + np.linalg.cholesky(S) @ eps).T)
    assert not hasattr(gp.model.ctx, "last_eps")


def test_posterior_sample_device_eps_layout_and_shape():
    X, y, Xt = _problem()
    gp = _gp(X, y)
    nt, ns = Xt.shape[0], 5
    s = dsm.posterior_sample(gp, Xt, ns, seed=9, device=True)
    assert s.shape == (ns, nt)
    want = datagen.normal(9, 0, nt * ns).reshape((nt, ns), order="F")
    assert np.array_equal(gp.model.ctx.last_eps, want)
    # the same law as the host path: on the double, which factorises with LAPACK too, the same bits
    assert np.array_equal(s, dsm.posterior_sample(gp, Xt, ns, seed=9))
    assert np.array_equal(dsm.posterior_sample(gp, Xt, ns, seed=9, with_noise=True, device=True),
                          dsm.posterior_sample(gp, Xt, ns, seed=9, with_noise=True))
    assert dsm.posterior_sample(gp, Xt, 0, device=True).shape == (0, nt)
    assert dsm.posterior_sample(gp, np.zeros((0, 2)), 3, device=True).shape == (3, 0)

    def failing(eps, with_noise=False, jitter=None):
        return np.full(eps.shape, np.nan, order="F"), np.array([3], dtype=np.int32)

    gp.model.ctx.predict_sample = failing
    with pytest.raises(np.linalg.LinAlgError):
        dsm.posterior_sample(gp, Xt, 2, device=True)


def test_leaf_samples_eps_layout_routes_and_values():
    X, y, Xt = _problem(N=400)
    m = _tree_model(X, y)
    ns = 4
    ptr, idx, draws, info = dsm.leaf_samples(m, Xt, ns, seed=21)
    hptr, hidx = dsm.tree.route_recursive(m.root, Xt)
    assert np.array_equal(ptr, hptr) and np.array_equal(idx, hidx)
    total = int(ptr[-1])
    assert draws.shape == (total, ns) and info.shape == (m.L,) and not np.any(info)
    want = datagen.normal(21, 0, total * ns).reshape((total, ns), order="F")
    assert np.array_equal(m.ctx.last_eps, want)
    mu, _ = m.ctx.predict_fetch()
    for l in range(m.L):
        a, b = int(ptr[l]), int(ptr[l + 1])
        if a == b:
            continue
        C = m.ctx.predict_cov_factor(l, b - a)
        assert np.array_equal(draws[a:b], mu[a:b, None] + C @ want[a:b])
    gp = _gp(*_problem()[:2])
    p1, i1, d1, f1 = dsm.leaf_samples(gp, _problem()[2], 3, seed=2)             # a single GP: one leaf, every row
    assert np.array_equal(p1, [0, 30]) and np.array_equal(i1, np.arange(30)) and d1.shape == (30, 3)
    assert np.array_equal(d1.T, dsm.posterior_sample(gp, _problem()[2], 3, seed=2, device=True))
    assert dsm.leaf_samples(m, Xt, 0)[2].shape == (total, 0)


def test_mixture_sample_composes_leaf_samples_along_the_chosen_children():
    X, y, Xt = _problem(N=400, nt=60)
    m = _tree_model(X, y)
    ns = 6
    ptr, idx, draws, _ = dsm.leaf_samples(m, Xt, ns, seed=4)
    out = dsm.mixture_sample(m, Xt, ns, seed=4)
    assert out.shape == (ns, Xt.shape[0])
    leaf_of_entry = np.repeat(np.arange(m.L), np.diff(ptr))
    nodes, choices = dmodel._mixture_choices(m.root, ns, 4)
    assert [int(nd.id.split("#")[1]) for nd in nodes] == sorted(int(nd.id.split("#")[1]) for nd in nodes) and len(nodes) >= 2
    for s in range(ns):
        chosen = dmodel._mixture_leaf_of_rows(m.root, Xt, nodes, choices[s])
        routed_sets = {}
        for r in range(Xt.shape[0]):
            ents = np.nonzero(idx == r)[0]
            # the value of the row is column s of exactly one of the leaves it is routed to: the chosen one
            hits = [e for e in ents if draws[e, s] == out[s, r]]
            assert len(hits) == 1 and leaf_of_entry[hits[0]] == chosen[r]
            # rows routed to the same set of leaves get the same leaf
            key = tuple(leaf_of_entry[ents])
            assert routed_sets.setdefault(key, chosen[r]) == chosen[r]
    # one-hot weights: the draw is leaf_samples at the selected leaves
    saved = [nd.logweights.copy() for nd in nodes]
    try:
        for nd in nodes:
            lw = np.full(len(nd.children), -np.inf)
            lw[len(nd.children) - 1] = 0.0
            nd.logweights = lw
        nodes1, ch1 = dmodel._mixture_choices(m.root, ns, 4)
        assert np.all(ch1 == np.array([len(nd.children) - 1 for nd in nodes1])[None, :])
        out1 = dsm.mixture_sample(m, Xt, ns, seed=4)
        chosen = dmodel._mixture_leaf_of_rows(m.root, Xt, nodes1, ch1[0])
        for r in range(Xt.shape[0]):
            e = int(ptr[chosen[r]] + np.searchsorted(idx[ptr[chosen[r]]:ptr[chosen[r] + 1]], r))
            assert idx[e] == r and np.array_equal(out1[:, r], draws[e, :])
    finally:
        for nd, lw in zip(nodes, saved):
            nd.logweights = lw


def test_selection_frequencies_of_a_two_level_tree():
    """A sum node over three sum nodes over three leaves each, weights (0.2, 0.3, 0.5) everywhere: over 20,000 draws the frequency
    of every child of every sum node lies within 5 sqrt(p (1 - p) / 20000) of p -- a 5 sigma binomial interval, false alarm
    below 1e-6 per child."""
    p = np.array([0.2, 0.3, 0.5])

    def leaf():
        return GPNode(np.arange(1), np.zeros(1), np.ones(1), None, 0, None, 0.0)

    root = GPSumNode()
    for _ in range(3):
        mid = GPSumNode(of_gps=True)
        for w in p:
            mid.add(leaf(), np.log(w))
        root.add(mid, 0.0)
    root.logweights = np.log(p) + 3.0          # not normalised: the law is exp(logweights) normalised
    n = 20000
    nodes, ch = dmodel._mixture_choices(root, n, seed=123)
    assert len(nodes) == 4 and ch.shape == (n, 4)
    for j in range(4):
        freq = np.bincount(ch[:, j], minlength=3) / n
        assert np.all(np.abs(freq - p) <= 5.0 * np.sqrt(p * (1.0 - p) / n)), (j, freq)
    # another seed is another stream; the same seed the same choices
    assert np.array_equal(ch, dmodel._mixture_choices(root, n, seed=123)[1])
    assert not np.array_equal(ch, dmodel._mixture_choices(root, n, seed=124)[1])


def test_refusals():
    X, y, Xt = _problem(N=400)
    for build in (dsm.buildPoE, dsm.buildBCM):
        pm = build(X, y, 3, M=40, kernel=dsm.IsoSE(np.log(0.4), 0.0), meanFun=None, logNoise=np.log(0.2), seed=5,
                   ctx=OracleSampleContext())
        with pytest.raises(TypeError):
            dsm.mixture_sample(pm, Xt, 2)
        ptr, idx, draws, info = dsm.leaf_samples(pm, Xt, 2)         # every expert draws at every row
        assert np.array_equal(np.diff(ptr), np.full(pm.L, Xt.shape[0])) and draws.shape == (pm.L * Xt.shape[0], 2)
    m = _tree_model(X, y)
    with pytest.raises(TypeError):
        dsm.posterior_sample(m, Xt, 2, device=True)
    with pytest.raises(ValueError):
        dsm.leaf_samples(m, Xt, -1)
    m.shard = types.SimpleNamespace(world=2, local=np.array([0, 1]))
    with pytest.raises(NotImplementedError):
        dsm.leaf_samples(m, Xt, 2)
    with pytest.raises(NotImplementedError):
        dsm.mixture_sample(m, Xt, 2)
    for cls in (hipabi.MultiContext, hipabi.StreamingContext):
        obj = cls.__new__(cls)                                      # no device: the refusal needs no state
        with pytest.raises(NotImplementedError):
            obj.predict_sample(np.zeros((4, 1)))
        with pytest.raises(NotImplementedError):
            obj.predict_cov_factor(0, 4)


def test_the_dependency_table_has_the_factors_below_the_prediction(tmp_path):
    exe = str(tmp_path / "ctx_state_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ctx_state_dump.cpp"), "-o", exe], check=True)
    table = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert table["sample_factors"]["parents"] == ["prediction"] and table["sample_factors"]["falls"] == []
    for p in ("prediction", "fit", "test", "plan"):
        assert "sample_factors" in table[p]["falls"], p
    for p in ("vt", "partial", "pred_gradients", "targets", "routing_tree"):
        assert "sample_factors" not in table[p]["falls"], p


def test_symbols_header_and_bindings():
    hdr = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    assert re.search(r"^int dsmgp_predict_sample\(dsmgp_ctx\* ctx, int32_t with_noise, double jitter,", hdr, flags=re.M)
    assert re.search(r"^int dsmgp_predict_cov_factor\(dsmgp_ctx\* ctx, int32_t leaf, double\* Lc_out", hdr, flags=re.M)
    import ctypes as C
    sig = hipabi.SIGNATURES["dsmgp_predict_sample"]
    assert sig[0] is C.c_int and len(sig[1]) == 10 and sig[1][2] is C.c_double and sig[1][5] is C.c_int32
    assert len(hipabi.SIGNATURES["dsmgp_predict_cov_factor"][1]) == 4
    assert hipabi.SAMPLE_JITTER == EPS
    # the Julia binding passes the scalar jitter by value, which its ccall table of test_host_cpu cannot express: the site is
    # written with @ccall, and its types are checked here against the prototype
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl")).read()
    m = re.search(r"@ccall \$fptr\((.*?)\)::Cint\)", src, flags=re.S)
    assert m and "sym(:dsmgp_predict_sample)" in src
    types_ = [a.rsplit("::", 1)[1].strip() for a in re.split(r",\s*(?![^()]*\))", m.group(1))]
    assert types_ == ["Ptr{Cvoid}", "Int32", "Float64", "Ptr{Float64}", "Int64", "Int32", "Ptr{Float64}", "Int64", "Ptr{Int32}",
                      "Ref{Float64}"]
    assert "predict_sample, predict_cov_factor" in src and "sym(:dsmgp_predict_cov_factor)" in src
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(hipabi.LIB_PATH)
    assert hasattr(lib, "dsmgp_predict_sample") and hasattr(lib, "dsmgp_predict_cov_factor")
