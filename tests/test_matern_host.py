"""The Matern kernels without a GPU: the parameter objects, the kind numbers shared with the C header, the dense restatement the
GPU tests compare against (tests/dense_gp.py on tests/dense_kernels.py) against the 50-digit references and the closed forms at r = 0 and r -> inf,
the model-side host paths (gradient rows, the rBCM prior), and the Julia glue's methods for them (julia/DSMGPHip.jl cannot be
executed here: its text is checked)."""
import os
import re

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import kernels
from pred_tolerance import EPS, mll_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "gp_matern.npz")
CLASSES = [(dsm.IsoMatern32, "ISO_MATERN32", 5, False), (dsm.IsoMatern52, "ISO_MATERN52", 6, False),
           (dsm.ArdMatern32, "ARD_MATERN32", 7, True), (dsm.ArdMatern52, "ARD_MATERN52", 8, True)]


@pytest.mark.parametrize("cls,name,kind,ard", CLASSES, ids=[c[1] for c in CLASSES])
def test_hyper_vector_layout_and_round_trip(cls, name, kind, ard):
    assert cls.kind == kind == getattr(kernels, "KIND_" + name)
    if ard:
        k = cls(np.log([0.5, 1.5, 2.0]), 0.3)
        assert k.loghyp().tolist() == list(np.log([0.5, 1.5, 2.0])) + [0.3]      # [logl_1..logl_D, logs]
        assert k.nparams() == 4 and k.dl.shape == (3,) and k.ds == 0.0
        k.set_loghyp(np.array([0.1, 0.2, 0.3, 7.0]))
        assert k.logl.tolist() == [0.1, 0.2, 0.3] and k.logs == 7.0
        c = k.copy()
        c.logl[0] = 9.0
        assert k.logl[0] == 0.1                                                  # copy owns its vector
        assert repr(k) == f"{cls.__name__}([0.1, 0.2, 0.3], 7.0)"
    else:
        k = cls(np.log(0.5), 0.3)
        assert k.loghyp().tolist() == [np.log(0.5), 0.3]                         # [logl, logs]
        assert k.nparams() == 2 and k.dl == 0.0 and k.ds == 0.0
        k.set_loghyp(np.array([0.1, 7.0]))
        assert k.logl == 0.1 and k.logs == 7.0
        assert repr(k) == f"{cls.__name__}(0.1, 7.0)"
    c = k.copy()
    assert type(c) is cls and c.kind == kind and c.loghyp().tolist() == k.loghyp().tolist()
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

    t = Table([Leaf(0, dsm.IsoSE(0.1, 0.2), -1.0), Leaf(1, dsm.ArdMatern52([0.3, 0.4], 0.5), -2.0),
               Leaf(2, dsm.IsoMatern32(0.6, 0.7), -3.0), Leaf(3, dsm.ArdLinear([0.8, 0.9]), -4.0)])
    assert M.getparams(t).tolist() == [0.1, 0.2, -1.0, 0.3, 0.4, 0.5, -2.0, 0.6, 0.7, -3.0, 0.8, 0.9, 0.0, -4.0]
    M.setparams(t, np.arange(1.0, 15.0))
    assert t.leaves[1].kernel.logl.tolist() == [4.0, 5.0] and t.leaves[1].kernel.logs == 6.0 and t.leaves[1].logNoise == 7.0
    assert t.leaves[2].kernel.logl == 8.0 and t.leaves[2].kernel.logs == 9.0 and t.leaves[2].logNoise == 10.0
    assert M.getparams(t).tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 0.0, 14.0]


def test_kinds_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "dsmgp_hip.h"), encoding="utf-8").read()
    for _, name, kind, _ in CLASSES:
        m = re.search(rf"#define\s+DSMGP_KIND_{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == kind == getattr(kernels, "KIND_" + name), name


def _golden():
    z = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in z.files})
    return [(n, {k.split("/")[1]: z[k] for k in z.files if k.startswith(n + "/")}) for n in names]


def test_golden_covers_every_kind_duplicates_and_spread_lengthscales():
    cases = dict(_golden())
    assert {int(c["kind"]) for c in cases.values()} == {5, 6, 7, 8}
    assert any(np.unique(c["X"], axis=0).shape[0] < c["X"].shape[0] for c in cases.values())      # duplicate points
    assert any(c["logl"].size > 1 and np.exp(np.ptp(c["logl"])) >= 99.9 for c in cases.values())  # l_d over two decades


@pytest.mark.parametrize("name,c", _golden(), ids=[n for n, _ in _golden()])
def test_dense_restatement_against_50_digit_references(name, c):
    import dense_kernels as dk
    from dense_gp import DenseGP
    kind = int(c["kind"])
    g = DenseGP(kind, dk.pack(kind, c["logl"], c["logs"], logNoise=c["logNoise"]), c["X"], c["y"], float(c["mean"]))
    assert g.info == 0
    cond = float(c["cond"])
    m = c["Kc"].shape[0]
    assert np.allclose(dk.value(kind, dk.pack(kind, c["logl"], c["logs"]), c["X"][:m], c["X"][:m]), c["Kc"], rtol=1e-13, atol=0)
    assert np.allclose(dk.value(kind, dk.pack(kind, c["logl"], c["logs"]), c["X"][:m], c["Xt"]), c["Kt"], rtol=1e-13, atol=0)
    assert abs(g.mll() - float(c["mll"])) <= mll_tol(float(c["mll"]), cond)
    mu, var = g.prediction(c["Xt"])
    tol = 64 * cond * EPS * max(1.0, float(np.max(np.abs(c["y"]))))
    assert np.max(np.abs(mu - c["mu"])) <= tol and np.max(np.abs(var - c["var"])) <= tol
    gd = g.grad()
    assert gd.size == c["grad"].size
    assert np.max(np.abs(gd - c["grad"])) <= 64 * cond * EPS * max(1.0, float(np.max(np.abs(c["grad"])))), (gd, c["grad"])


@pytest.mark.parametrize("kind", [5, 6, 7, 8])
def test_closed_forms_at_r_zero_and_r_to_infinity(kind):
    """k(x, x) = sigma^2 exactly; far apart k -> 0 with the nu-specific tail; at one s the textbook polynomial; the iso kind
    is the ARD kind with equal length-scales."""
    import dense_kernels as dk
    from dense_kernels import two_nu

    def is_ard(kind):
        return kind in dk.ARD
    D, ls = 3, 0.4
    ll = np.log([0.7] * (D if is_ard(kind) else 1))
    x = np.array([[0.1, 0.2, 0.3]])
    assert dk.value(kind, dk.pack(kind, ll, ls), x, x)[0, 0] == np.exp(2 * ls)
    far = x + 1e3
    assert dk.value(kind, dk.pack(kind, ll, ls), x, far)[0, 0] == 0.0
    # s = sqrt(2 nu) r with r = |a - b| / l
    b = x + np.array([[0.3, -0.1, 0.2]])
    r = np.sqrt(np.sum((x - b) ** 2)) / 0.7
    s = np.sqrt(two_nu(kind)) * r
    p = 1 + s if two_nu(kind) == 3.0 else 1 + s + s * s / 3
    assert abs(dk.value(kind, dk.pack(kind, ll, ls), x, b)[0, 0] - np.exp(2 * ls) * p * np.exp(-s)) <= 1e-15
    # tail: k / sigma^2 = e^-s (1 + s [+ s^2 / 3]) at s = 30
    b30 = x + np.array([[30.0 * 0.7 / np.sqrt(two_nu(kind)), 0.0, 0.0]])
    tail = (31.0 if two_nu(kind) == 3.0 else 1 + 30 + 300.0) * np.exp(-30.0)
    assert abs(dk.value(kind, dk.pack(kind, ll, 0.0), x, b30)[0, 0] - tail) <= 1e-12 * tail
    if not is_ard(kind):
        assert np.array_equal(dk.value(kind, dk.pack(kind, ll, ls), x, b),
                              dk.value(kind + 2, dk.pack(kind + 2, np.full(D, ll[0]), ls), x, b))


@pytest.mark.parametrize("kind", [5, 6, 7, 8])
def test_dense_gradients_are_finite_at_duplicate_points_and_match_finite_differences(kind):
    import dense_kernels as dk
    from dense_gp import DenseGP
    from deepstructuredmixtures_amd.datagen import uniform, normal
    n, D = 60, 2
    X = uniform(31, 0, n * D).reshape((n, D), order="F")
    X[50:] = X[:10]                                             # s = 0 off the diagonal
    y = np.sin(3 * X[:, 0]) + 0.1 * normal(32, 0, n)
    ll = np.log([0.4, 0.9]) if kind in dk.ARD else np.log([0.6])
    h = np.concatenate([ll, [0.1, np.log(0.3)]])
    g = DenseGP(kind, h, X, y, 0.0).grad()
    assert np.all(np.isfinite(g))
    e = 1e-6
    for j in range(h.size):
        hp, hm = h.copy(), h.copy()
        hp[j] += e
        hm[j] -= e
        fd = (DenseGP(kind, hp, X, y, 0.0).mll() - DenseGP(kind, hm, X, y, 0.0).mll()) / (2 * e)
        assert abs(fd - g[j]) <= 1e-6 * max(1.0, abs(fd)), (j, fd, g[j])


def test_gradient_rows_and_rbcm_prior_on_the_host():
    """updategradients' row layout (iso: scalar dl, ARD: a D-vector) and _prior_diag = sigma^2 for every Matern kind."""
    from deepstructuredmixtures_amd import model as M
    xt = np.ones((5, 3))
    for cls, _, kind, ard in CLASSES:
        k = cls(np.log([0.5] * 3) if ard else np.log(0.5), 0.2)

        class Leaf:
            kernel = k
        assert np.array_equal(M._prior_diag(Leaf, xt), np.full(5, np.exp(0.4)))
    src = open(os.path.join(ROOT, "deepstructuredmixtures_amd", "model.py"), encoding="utf-8").read()
    body = src[src.index("def updategradients"):src.index("def grad_mll")]
    assert "KIND_ARD_MATERN32, KIND_ARD_MATERN52" in body


def test_julia_glue_maps_the_matern_types():
    """Four types (IsoSE's fields for the iso kinds, ArdSE's for the ARD ones), kinds 5-8 as in the header, loghyp with the
    IsoSE / ArdSE layouts, the reference methods GaussianProcess and params / setparams! call on a kernel, and gradients written
    into k.∂ℓ (in place for the ARD types) and k.∂σ."""
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    for cls, name, kind, ard in CLASSES:
        t = cls.__name__
        m = re.search(rf"(?m)^kind\(::{t}\) = Int32\((\d+)\)", src)
        assert m and int(m.group(1)) == kind, t
        sup = "ArdKernel" if ard else "IsoKernel"
        st = re.search(rf"(?ms)^mutable struct {t}\{{T<:AbstractFloat\}} <: DeepStructuredMixtures\.{sup}\n(.*?)^end", src)
        assert st and re.findall(r"(\S+)::", st.group(1)) == ["logℓ", "logσ", "∂ℓ", "∂σ"], t
        assert re.search(rf"(?m)^{t}\(logℓ, logσ\) = {t}\(logℓ, logσ, zero\(logℓ\), zero\(logσ\)\)", src), t
        assert re.search(rf"(?m)^export .*\b{t}\b", src), t
    assert re.search(r"(?m)^const IsoMatern = Union\{IsoMatern32,IsoMatern52\}", src)
    assert re.search(r"(?m)^const ArdMatern = Union\{ArdMatern32,ArdMatern52\}", src)
    assert re.search(r"(?m)^loghyp\(k::IsoMatern, ln\) = Float64\[k\.logℓ, k\.logσ, ln\]", src)
    assert re.search(r"(?m)^loghyp\(k::ArdMatern, ln\) = Float64\[k\.logℓ\.\.\., k\.logσ, ln\]", src)
    for meth in ("getvariance", "getstd", "setvariance!", "getlengthscales", "setlengthscale!", "getdistancematrix"):
        assert re.search(rf"(?m)^DeepStructuredMixtures\.{re.escape(meth)}\(k::(Union\{{IsoMatern,ArdMatern\}}|IsoMatern)", src), meth
        assert re.search(rf"(?m)^DeepStructuredMixtures\.{re.escape(meth)}\(k::(Union\{{IsoMatern,ArdMatern\}}|ArdMatern)", src), meth
    body = src[src.index("function fetchgradients!"):]
    body = body[:body.index("\nend\n")]
    assert body.count("k isa ArdMatern") == 2 and "k.∂ℓ[:] = g[1:nl, l]" in body and "k.∂ℓ = g[1, l]" in body
