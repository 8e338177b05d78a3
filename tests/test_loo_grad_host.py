"""CPU tests of the LOO-gradient references and host logic: the float64 dense helper (tests/loo_grad_dense.py) against the
50-digit fixture (tests/golden/gp_loo_grad.npz), against central differences of loo_dense.loo_dense and against the literal
form of GPML eq. 5.13; loo_objective / grad_loo on hand-made trees with injected leaf values; grad_mll unchanged; the
prototypes."""
import os
import re

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_kernels as dk
import loo_grad_dense as lgd
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = lgd.load_cases()


def test_fixture_covers_the_cases_the_feature_names():
    ns = {c["X"].shape[0] for c in CASES.values()}
    Ds = {c["X"].shape[1] for c in CASES.values()}
    assert {1, 2, 127, 128, 129, 300} <= ns and {1, 8, 40} <= Ds
    assert {c["kind"] for c in CASES.values()} == set(range(9))
    assert all(c["X"].shape[1] <= 35 for c in CASES.values() if c["kind"] == 1)
    assert all(c["X"].shape[0] <= 64 for c in CASES.values() if c["X"].shape[1] == 40)
    assert any(abs(c["mean"] - float(np.mean(c["y"]))) > 0.1 for c in CASES.values())
    assert max(float(np.max(np.abs(c["y"]))) for c in CASES.values()) > 500.0
    assert {c["kind"] for c in CASES.values() if c["weak"]} == {0, 2}
    for c in CASES.values():
        if c["weak"]:       # sigma^2 / c = 1e-8 (IsoLinear: 1 / l^2 in the place of sigma^2)
            s2 = np.exp(2.0 * c["loghyp"][1]) if c["kind"] == 0 else np.exp(-2.0 * c["loghyp"][0])
            assert abs(s2 / (np.exp(2.0 * c["logNoise"]) + 1e-8) / 1e-8 - 1.0) < 1e-9
    assert all(c["cond"] <= 1e6 for c in CASES.values())
    assert os.path.getsize(os.path.join(GOLDEN, "gp_loo_grad.npz")) <= os.path.getsize(os.path.join(GOLDEN, "gp_pred.npz"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_helper_against_50_digits(name):
    """The condition on the fixture: the float64 helper stays within 0.05 of the tolerance on every component; its summed lpd
    agrees with the 50-digit one."""
    c = CASES[name]
    noise = float(np.exp(2.0 * c["logNoise"]))
    K = dk.value(c["kind"], c["loghyp"], c["X"], c["X"])
    g = lgd.loo_grad_dense(K, dk.d_hyper(c["kind"], c["loghyp"], c["X"])[1], noise, c["y"], c["mean"])
    assert g.shape == c["grad"].shape
    r = float(np.max(np.abs(g - c["grad"]) / lgd.tolerance(c, c["grad"], K)))
    print(f"\n{name}: cond {c['cond']:.3g}, dense err/tol {r:.3g}")
    assert r <= 0.05, (name, r)
    assert abs(lgd.lpd_sum(K, noise, c["y"], c["mean"]) - c["lpd"]) <= 64.0 * c["cond"] * lgd.EPS * max(1.0, abs(c["lpd"]))


def _random_case(kind, n, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, D))
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n) + 0.5
    nl = D if kind in (1, 3, 4, 7, 8) else 1
    loghyp = np.concatenate([np.log(rng.uniform(0.6, 1.5, size=nl)), [0.0 if kind in (2, 3) else rng.uniform(-0.3, 0.3)]])
    return X, y, float(np.mean(y)) + 0.15, loghyp, float(np.log(0.3))


@pytest.mark.parametrize("kind", range(9))
def test_dense_helper_against_central_differences_and_the_literal_form(kind):
    """Fresh random cases of every kind: the M form against float64 central differences of loo_dense.loo_dense
    (2e-6 max(1, |fd|), the bound of the existing finite-difference tests) and against eq. 5.13 as printed."""
    X, y, mean, loghyp, logNoise = _random_case(kind, 40 + 3 * kind, 1 + kind % 3, 100 + kind)

    def lpd(h):
        return lgd.lpd_sum(dk.value(kind, h[:-1], X, X), float(np.exp(2.0 * h[-1])), y, mean)

    h0 = np.concatenate([loghyp, [logNoise]])
    noise = float(np.exp(2.0 * logNoise))
    K = dk.value(kind, loghyp, X, X)
    dKs = dk.d_hyper(kind, loghyp, X)[1]
    g = lgd.loo_grad_dense(K, dKs, noise, y, mean)
    lit = lgd.loo_grad_literal(K, dKs, noise, y, mean)
    assert np.max(np.abs(g - lit)) <= 1e-10 * max(1.0, float(np.max(np.abs(lit))))
    for j in range(h0.size):
        hp, hm = h0.copy(), h0.copy()
        hp[j] += 1e-5
        hm[j] -= 1e-5
        fd = (lpd(hp) - lpd(hm)) / 2e-5
        assert abs(g[j] - fd) <= 2e-6 * max(1.0, abs(fd)), (kind, j, g[j], fd)
    if kind in (2, 3):
        assert g[-2] == 0.0


# ------------------------------------------------------------------------------------- the tree recursions

def _problem(N, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, D))
    return X, np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(N)


def _models():
    X, y = _problem(1500, 2, 61)
    yield dsm.buildDSMGP(X, y, 3, 3, M=40, D=2, kernel=dsm.IsoSE(0.0, 0.0), fit_now=False, seed=3)
    yield dsm.buildDSMGP(X, y, 2, 3, M=40, D=2, kernel=[dsm.IsoSE(0.0, 0.0), dsm.IsoLinear(0.0)], fit_now=False, seed=4)


def _inject(m, rng):
    """Synthetic leaf functions lpd_l(h) = a_l + sum_j sin(f_lj h_chunk(l),j): values and analytic leaf gradients at h."""
    off, c = {}, 0
    for lf in m.kernel_table():
        off[lf.kernelid] = (c, lf.kernel.nparams() + 1)
        c += lf.kernel.nparams() + 1
    stride = max(n for _, n in off.values())
    a = -20.0 * rng.random(m.L) - 5.0
    f = rng.uniform(0.5, 2.0, size=(m.L, stride))

    def values(h):
        v, g = np.zeros(m.L), np.zeros((m.L, stride))
        for l, lf in enumerate(m.leaves):
            c0, nn = off[lf.kernelid]
            v[l] = a[l] + np.sum(np.sin(f[l, :nn] * h[c0:c0 + nn]))
            g[l, :nn] = f[l, :nn] * np.cos(f[l, :nn] * h[c0:c0 + nn])
        return v, g

    return values


def test_loo_objective_and_grad_loo_against_central_differences_of_the_recursion():
    rng = np.random.default_rng(7)
    some_sum_over_kernels = False
    for m in _models():
        from deepstructuredmixtures_amd.tree import ordered_nodes
        some_sum_over_kernels |= any(n.kind == "sum" and n.of_gps for n in ordered_nodes(m.root))
        values = _inject(m, rng)
        h0 = rng.uniform(-0.5, 0.5, size=dsm.getparams(m).size)
        m.leaf_lpd, m.leaf_grad = values(h0)
        assert dsm.loo_objective(m, lpd=m.leaf_lpd) == dmodel._value_table(m, m.leaf_lpd)[m.root.id]
        m.leaf_mll = m.leaf_lpd.copy()
        assert dsm.loo_objective(m, lpd=m.leaf_lpd) == dmodel.mll_table(m)[m.root.id]      # the recursion of mll
        g = dsm.grad_loo(m)
        assert g.size == h0.size
        for j in range(h0.size):
            hp, hm = h0.copy(), h0.copy()
            hp[j] += 1e-6
            hm[j] -= 1e-6
            fd = (dsm.loo_objective(m, lpd=values(hp)[0]) - dsm.loo_objective(m, lpd=values(hm)[0])) / 2e-6
            assert abs(g[j] - fd) <= 1e-7 * max(1.0, abs(fd)), (j, g[j], fd)
    assert some_sum_over_kernels


def _grad_mll_parent(model, leaf_weights=None):
    """The recursion of grad_mll as the parent commit has it (kept here to pin its results to the bit)."""
    tab = dmodel.mll_table(model)
    logS = tab[model.root.id]
    grad = np.zeros(dsm.getparams(model).size)

    def rec(node, dparent, lrho, g):
        if node.kind == "gp":
            w = np.exp(-logS + lrho + tab[node.id] + dparent)
            if leaf_weights is not None:
                w = w * leaf_weights[node.leaf]
            g += model.leaf_grad[node.leaf][: g.size] * w
        elif node.kind == "split":
            for c in node.children:
                rec(c, dparent + (tab[node.id] - tab[c.id]), lrho, g)
        elif node.of_gps:
            c0 = 0
            for c in node.children:
                nn = c.kernel.nparams() + 1
                rec(c, dparent, lrho, g[c0:c0 + nn])
                c0 += nn
        else:
            K = len(node.children)
            for c in node.children:
                rec(c, -np.log(K) + dparent, np.log(K) + lrho, g)

    rec(model.root, 0.0, 0.0, grad)
    return grad


def test_grad_mll_is_bit_identical_to_the_parent_recursion():
    rng = np.random.default_rng(8)
    for m in _models():
        values = _inject(m, rng)
        m.leaf_mll, m.leaf_grad = values(rng.uniform(-0.5, 0.5, size=dsm.getparams(m).size))
        w = rng.random(m.L)
        for lw in (None, w):
            a, b = dsm.grad_mll(m, lw), _grad_mll_parent(m, lw)
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_objective_argument_is_checked_and_a_streaming_context_refuses():
    X, y = _problem(300, 2, 62)
    m = dsm.buildDSMGP(X, y, 2, 2, M=40, D=1, kernel=dsm.IsoSE(0.0, 0.0), fit_now=False, seed=3)
    with pytest.raises(ValueError):
        dsm.train(m, objective="elbo", iterations=1)
    with pytest.raises(ValueError):
        dsm.updategradients(m, objective="elbo")
    with pytest.raises(hipabi.DsmgpError) as ei:
        hipabi.StreamingContext.loo_gradients(object.__new__(hipabi.StreamingContext), 3)
    assert ei.value.code == hipabi.E_STATE

    class Streaming:                    # what train() recognises a factor-and-discard context by; any call on it would raise
        want_gradients = 0
        groups = None

    m._ctx = Streaming()
    h0 = dsm.getparams(m).copy()
    with pytest.raises(hipabi.DsmgpError) as ei:
        dsm.train(m, objective="loo", iterations=1)
    assert ei.value.code == hipabi.E_STATE and "streaming" in str(ei.value)
    assert np.array_equal(dsm.getparams(m), h0) and Streaming.want_gradients == 0      # refused before any side effect


# ------------------------------------------------------------------------------------- the prototypes

def test_header_export_and_julia_prototype():
    assert "dsmgp_loo_gradients" in hipabi.SIGNATURES
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int dsmgp_loo_gradients(dsmgp_ctx* ctx, double* grad_out , int32_t stride, double* lpd_out , double* seconds );" in flat)
    assert "#define DSMGP_N_TIMINGS 21" in header
    julia = open(os.path.join(ROOT, "julia", "DSMGPHip.jl")).read()
    assert "ccall(sym(:dsmgp_loo_gradients), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}, Ref{Float64})" in julia
    assert "loo_gradients" in julia.split("export", 1)[1]
