"""ArdSEProduct without a GPU: the parameter object, the kind number shared with the C header, the dense restatement the GPU
tests compare against (tests/dense_gp.py on tests/dense_kernels.py) against the 50-digit references and the oracle's IsoSE, and the Julia
glue's methods for it (julia/DSMGPHip.jl cannot be executed here: its text is checked)."""
import os
import re

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import kernels
from pred_tolerance import EPS, mll_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gp_ardse_product.npz")
KIND = kernels.KIND_ARD_SE_PRODUCT


def test_hyper_vector_layout_and_round_trip():
    k = dsm.ArdSEProduct(np.log([0.5, 1.5, 2.0]), 0.3)
    assert k.kind == KIND == 4
    assert k.loghyp().tolist() == list(np.log([0.5, 1.5, 2.0])) + [0.3]      # [logl_1..logl_D, logs]
    assert k.nparams() == 4 and k.dl.shape == (3,) and k.ds == 0.0
    k.set_loghyp(np.array([0.1, 0.2, 0.3, 7.0]))
    assert k.logl.tolist() == [0.1, 0.2, 0.3] and k.logs == 7.0
    c = k.copy()
    c.logl[0] = 9.0
    assert k.logl[0] == 0.1                                                  # copy owns its vector
    assert repr(k) == "ArdSEProduct([0.1, 0.2, 0.3], 7.0)"
    assert isinstance(k, dsm.KernelFunction)


def test_parameters_through_getparams_setparams_with_a_mixed_table():
    from deepstructuredmixtures_amd import model as M

    class Leaf:
        def __init__(self, kid, kern, ln):
            self.kernelid, self.kernel, self.logNoise = kid, kern, ln

    class Table:
        def __init__(self, leaves):
            self.leaves = leaves

        def kernel_table(self):
            return self.leaves

    t = Table([Leaf(0, dsm.IsoSE(0.1, 0.2), -1.0), Leaf(1, dsm.ArdSEProduct([0.3, 0.4], 0.5), -2.0),
               Leaf(2, dsm.ArdLinear([0.6, 0.7]), -3.0)])
    assert M.getparams(t).tolist() == [0.1, 0.2, -1.0, 0.3, 0.4, 0.5, -2.0, 0.6, 0.7, 0.0, -3.0]
    M.setparams(t, np.arange(1.0, 12.0))
    assert t.leaves[1].kernel.logl.tolist() == [4.0, 5.0] and t.leaves[1].kernel.logs == 6.0 and t.leaves[1].logNoise == 7.0
    assert M.getparams(t).tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 0.0, 11.0]


def test_kind_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "dsmgp_hip.h"), encoding="utf-8").read()
    m = re.search(r"#define\s+DSMGP_KIND_ARD_SE_PRODUCT\s+(\d+)", hdr)
    assert m and int(m.group(1)) == kernels.KIND_ARD_SE_PRODUCT


def _golden():
    z = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in z.files})
    return [(n, {k.split("/")[1]: z[k] for k in z.files if k.startswith(n + "/")}) for n in names]


@pytest.mark.parametrize("name,c", _golden(), ids=[n for n, _ in _golden()])
def test_dense_restatement_against_50_digit_references(name, c):
    import dense_kernels as dk
    from dense_gp import DenseGP
    g = DenseGP(4, dk.pack(4, c["logl"], c["logs"], logNoise=c["logNoise"]), c["X"], c["y"], float(c["mean"]))
    assert g.info == 0
    cond = float(c["cond"])
    m = c["Kc"].shape[0]
    assert np.allclose(dk.value(4, dk.pack(4, c["logl"], c["logs"]), c["X"][:m], c["X"][:m]), c["Kc"], rtol=1e-13, atol=0)
    assert abs(g.mll() - float(c["mll"])) <= mll_tol(float(c["mll"]), cond)
    mu, var = g.prediction(c["Xt"])
    tol = 64 * cond * EPS * max(1.0, float(np.max(np.abs(c["y"]))))
    assert np.max(np.abs(mu - c["mu"])) <= tol and np.max(np.abs(var - c["var"])) <= tol
    gd = g.grad()
    assert np.max(np.abs(gd - c["grad"])) <= 64 * cond * EPS * max(1.0, float(np.max(np.abs(c["grad"])))), (gd, c["grad"])


def test_dense_restatement_with_equal_lengthscales_is_the_oracle_iso_se():
    """With every l_d = l: the oracle's IsoSE(l, s) in K, log-marginal and moments; sum_d dl_d * sigma = IsoSE's dl and
    ds * sigma = IsoSE's ds (the reference's factor sigma)."""
    import dense_kernels as dk
    from dense_gp import DenseGP
    from oracle import gp as ogp
    from deepstructuredmixtures_amd.datagen import uniform, normal
    n, D = 300, 3
    X = uniform(7, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3 * X[:, 0]) + 0.1 * normal(8, 0, n)
    Xt = uniform(9, 0, 40 * D).reshape((40, D), order="F")
    ll, ls, ln, m = np.log(0.5), 0.2, np.log(0.3), float(np.mean(y))
    g = DenseGP(4, dk.pack(4, np.full(D, ll), ls, logNoise=ln), X, y, m)
    k = ogp.make_kernel(0, np.array([ll, ls]))
    o = ogp.GaussianProcess(X, y, m, k, ln, exact_dist=True).update_cholesky()
    Ko = ogp.kernelmatrix(k, X, Xt)
    assert np.max(np.abs(dk.value(4, dk.pack(4, np.full(D, ll), ls), X, Xt) - Ko)) <= 1e-14 * np.max(np.abs(Ko))
    assert abs(g.mll() - o.mll()) <= 1e-11 * abs(o.mll())
    mu, var = g.prediction(Xt)
    mo, vo = o.prediction(Xt)
    assert np.allclose(mu, mo, rtol=1e-10, atol=1e-12) and np.allclose(var, vo, rtol=1e-9, atol=1e-12)
    gd, go = g.grad(), o.grad()
    s = np.exp(ls)
    assert abs(np.sum(gd[:D]) * s - go[0]) <= 1e-9 * max(1.0, abs(go[0]))
    assert abs(gd[D] * s - go[1]) <= 1e-9 * max(1.0, abs(go[1]))
    assert abs(gd[D + 1] - go[2]) <= 1e-9 * max(1.0, abs(go[2]))


def test_julia_glue_maps_ardse_product():
    """An ArdSEProduct type with ArdSE's fields, kind 4 as in the header, loghyp with the ArdSE layout, the reference methods
    GaussianProcess and params / setparams! call on a kernel, and gradients written in place into k.∂ℓ and k.∂σ."""
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    m = re.search(r"(?m)^kind\(::ArdSEProduct\) = Int32\((\d+)\)", src)
    assert m and int(m.group(1)) == kernels.KIND_ARD_SE_PRODUCT
    assert re.search(r"(?m)^loghyp\(k::ArdSEProduct, ln\) = Float64\[k\.logℓ\.\.\., k\.logσ, ln\]", src)
    st = re.search(r"(?ms)^mutable struct ArdSEProduct\{T<:AbstractFloat\} <: DeepStructuredMixtures\.ArdKernel\n(.*?)^end", src)
    assert st and re.findall(r"(\S+)::", st.group(1)) == ["logℓ", "logσ", "∂ℓ", "∂σ"]
    for meth in ("getvariance", "getstd", "setvariance!", "getlengthscales", "setlengthscale!", "getdistancematrix"):
        assert re.search(rf"(?m)^DeepStructuredMixtures\.{re.escape(meth)}\(k::ArdSEProduct", src), meth
    body = src[src.index("function fetchgradients!"):]
    body = body[:body.index("\nend\n")]
    assert body.count("k isa Union{ArdSE,ArdLinear} || k isa ArdSEProduct") == 2 and "k.∂ℓ[:] = g[1:nl, l]" in body
    assert "k isa Union{IsoLinear,ArdLinear} || (k.∂σ = g[nl + 1, l])" in body
