"""Host-side tests of the rational quadratic kernels (kinds 9 and 10), no GPU: the kernel classes and their hyper-vector layout,
getparams / setparams, the kind constants against the header, and the dense restatement of tests/dense_gp.py -- the reference of
tests/test_rq_gpu.py -- against the 50-digit references of tests/golden/gp_rq.npz, closed forms, central differences of its own log-marginal, LOO density and predictions, and the
large-alpha bound against the product-form squared exponential."""
import os
import re

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import kernels
from deepstructuredmixtures_amd import model as M
import dense_kernels as dk
import loo_dense
import loo_grad_dense as lgd
import predgrad_dense as pgd
from dense_gp import DenseGP
from pred_tolerance import EPS, mll_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO_RQ, ARD_RQ = KINDS = dk.RQ


def is_ard(kind):
    return kind in dk.ARD


def load_cases():
    """The cases of tests/golden/gp_rq.npz (tests/golden/make_rq_golden.py), name -> dict of arrays and Python scalars."""
    return {name: {f: v if v.ndim else v.item() for f, v in c.items()} for name, c in dk.load_cases("gp_rq.npz").items()}


def test_hyper_vector_layout_and_round_trip():
    assert dsm.IsoRQ.kind == kernels.KIND_ISO_RQ == ISO_RQ and dsm.ArdRQ.kind == kernels.KIND_ARD_RQ == ARD_RQ
    k = dsm.ArdRQ(np.log([0.5, 1.5, 2.0]), 0.7, 0.3)
    assert k.loghyp().tolist() == list(np.log([0.5, 1.5, 2.0])) + [0.7, 0.3]     # [logl_1..logl_D, loga, logs]
    assert k.nparams() == 5 and k.dl.shape == (3,) and k.da == 0.0 and k.ds == 0.0
    k.set_loghyp(np.array([0.1, 0.2, 0.3, 5.0, 7.0]))
    assert k.logl.tolist() == [0.1, 0.2, 0.3] and k.loga == 5.0 and k.logs == 7.0
    c = k.copy()
    c.logl[0] = 9.0
    assert k.logl[0] == 0.1 and type(c) is dsm.ArdRQ and c.loga == 5.0
    assert repr(k) == "ArdRQ([0.1, 0.2, 0.3], 5.0, 7.0)"
    k = dsm.IsoRQ(np.log(0.5), 0.7, 0.3)
    assert k.loghyp().tolist() == [np.log(0.5), 0.7, 0.3]                        # [logl, loga, logs]
    assert k.nparams() == 3 and k.dl == 0.0 and k.da == 0.0 and k.ds == 0.0
    k.set_loghyp(np.array([0.1, 5.0, 7.0]))
    assert (k.logl, k.loga, k.logs) == (0.1, 5.0, 7.0) and repr(k) == "IsoRQ(0.1, 5.0, 7.0)"
    assert k.copy().loghyp().tolist() == k.loghyp().tolist() and isinstance(k, dsm.KernelFunction)


def test_parameters_through_getparams_setparams_with_a_mixed_table():
    class Leaf:
        def __init__(self, kid, kern, ln):
            self.kernelid, self.kernel, self.logNoise = kid, kern, ln

    class Table:
        def __init__(self, leaves):
            self.leaves = leaves

        def kernel_table(self):
            return self.leaves

    t = Table([Leaf(0, dsm.IsoSE(0.1, 0.2), -1.0), Leaf(1, dsm.ArdRQ([0.3, 0.4], 0.45, 0.5), -2.0),
               Leaf(2, dsm.IsoRQ(0.6, 0.65, 0.7), -3.0)])
    assert M.getparams(t).tolist() == [0.1, 0.2, -1.0, 0.3, 0.4, 0.45, 0.5, -2.0, 0.6, 0.65, 0.7, -3.0]
    M.setparams(t, np.arange(1.0, 13.0))
    k1, k2 = t.leaves[1].kernel, t.leaves[2].kernel
    assert k1.logl.tolist() == [4.0, 5.0] and (k1.loga, k1.logs, t.leaves[1].logNoise) == (6.0, 7.0, 8.0)
    assert (k2.logl, k2.loga, k2.logs, t.leaves[2].logNoise) == (9.0, 10.0, 11.0, 12.0)
    assert M.getparams(t).tolist() == list(np.arange(1.0, 13.0))


def test_kinds_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "dsmgp_hip.h"), encoding="utf-8").read()
    for name, kind in (("ISO_RQ", 9), ("ARD_RQ", 10)):
        m = re.search(rf"#define\s+DSMGP_KIND_{name}\s+(\d+)", hdr)
        assert m and int(m.group(1)) == kind == getattr(kernels, "KIND_" + name), name


def test_prior_variance_on_the_host():
    class Leaf:
        kernel = dsm.ArdRQ([0.1, 0.2], 0.3, 0.4)

    xt = np.ones((5, 2))
    assert np.array_equal(M._prior_diag(Leaf, xt), np.full(5, np.exp(0.8)))
    assert np.array_equal(M._prior_diag_grad(Leaf, xt), np.zeros((5, 2)))


CASES = load_cases()


def test_golden_covers_the_cases_the_feature_names():
    cs = CASES.values()
    assert {c["kind"] for c in cs} == {9, 10}
    assert {1, 2, 300} <= {c["X"].shape[0] for c in cs} and max(c["X"].shape[0] for c in cs) == 300
    assert {1, 3, 8} == {c["X"].shape[1] for c in cs}
    for kind in KINDS:
        assert {round(float(np.exp(c["loga"])), 12) for c in cs if c["kind"] == kind} == {0.3, 2.0, 50.0}
        assert any(np.unique(c["X"], axis=0).shape[0] < c["X"].shape[0] for c in cs if c["kind"] == kind)  # duplicate points
    assert any(c["logl"].size > 1 and np.exp(np.ptp(c["logl"])) >= 99.9 for c in cs)                      # l_d over two decades
    assert all(any(np.array_equal(c["Xt"][0], x) for x in c["X"]) for c in cs)                            # x_t on a training point
    assert all(c["cond"] <= 1e6 for c in cs)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gp_rq.npz")) < 500_000


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_restatement_against_50_digit_references(name):
    """Every quantity of the fixture at the tolerances of the Matern host test (K corners 1e-13 relative; mll_tol; moments and
    log-marginal gradient 64 cond_2(K_y) eps of their scale), of the LOO host tests (loo_dense.loo_tol at 0.01,
    loo_grad_dense.tolerance at 0.05) and of the input-gradient host test (predgrad_dense.tolerances, with the scales of the
    squared exponential at the same length-scales and sigma: |dk/dx_d| <= k |x_d - x'_d| / l_d^2 there and here)."""
    c = CASES[name]
    kind, cond, D = c["kind"], c["cond"], c["X"].shape[1]
    g = DenseGP(kind, dk.pack(kind, c["logl"], c["logs"], c["loga"], c["logNoise"]), c["X"], c["y"], c["mean"])
    assert g.info == 0
    m = c["Kc"].shape[0]
    assert np.allclose(dk.value(kind, dk.pack(kind, c["logl"], c["logs"], c["loga"]), c["X"][:m], c["X"][:m]), c["Kc"], rtol=1e-13, atol=0)
    assert np.allclose(dk.value(kind, dk.pack(kind, c["logl"], c["logs"], c["loga"]), c["X"][:m], c["Xt"]), c["Kt"], rtol=1e-13, atol=0)
    assert abs(g.mll() - c["mll"]) <= mll_tol(c["mll"], cond)
    mu, var = g.prediction(c["Xt"])
    tol = 64 * cond * EPS * max(1.0, float(np.max(np.abs(c["y"]))))
    assert np.max(np.abs(mu - c["mu"])) <= tol and np.max(np.abs(var - c["var"])) <= tol
    gd = g.grad()
    assert gd.size == c["grad"].size == (D if is_ard(kind) else 1) + 3
    r_g = float(np.max(np.abs(gd - c["grad"])) / (64 * cond * EPS * max(1.0, float(np.max(np.abs(c["grad"]))))))
    assert r_g <= 1.0, (gd, c["grad"])
    noise, kss = float(np.exp(2.0 * c["logNoise"])), np.full(c["y"].size, np.exp(2.0 * c["logs"]))
    lmu, lvar, lsum = g.loo()
    d = 1.0 / lvar
    lpd = -(np.log(2.0 * np.pi) + np.log(lvar) + (g.alpha / d) ** 2 / lvar) / 2.0
    tm, tv, tl, ts = loo_dense.loo_tol(c["y"], c["loo_mu"], c["loo_var"], kss, noise)
    r_loo = max(np.max(np.abs(lmu - c["loo_mu"]) / tm), np.max(np.abs(lvar - c["loo_var"]) / tv), np.max(np.abs(lpd - c["lpd"]) / tl),
                abs(lsum - c["lpd_sum"]) / ts)
    assert r_loo <= 0.01, (name, r_loo)
    assert abs(lsum - c["lpd_sum"]) <= 64.0 * cond * EPS * max(1.0, abs(c["lpd_sum"]))
    lg = g.loo_grad()
    assert lg.shape == c["loo_grad"].shape
    r_lg = float(np.max(np.abs(lg - c["loo_grad"]) / lgd.tolerance(dict(c, weak=False), c["loo_grad"])))
    assert r_lg <= 0.05, (name, r_lg)
    dmu, dvar = g.input_gradients(c["Xt"])
    he = np.append(np.broadcast_to(c["logl"], (D,)), c["logs"])
    tdm, tdv = pgd.tolerances(4, he, c["logNoise"], c["X"], c["y"], c["Xt"], c["dmu"], c["dvar"])
    r_in = max(float(np.max(np.abs(dmu - c["dmu"]) / tdm)), float(np.max(np.abs(dvar - c["dvar"]) / tdv)))
    assert r_in <= 1.0, (name, r_in)
    print(f"\n{name}: cond {cond:.3g}, dense err/tol grad {r_g:.3g} loo {r_loo:.3g} loo grad {r_lg:.3g} input grad {r_in:.3g}")


def _case(kind, n, D, seed, dup=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, D))
    X[n - dup:] = X[:dup]                                      # duplicate training points: w = 0 off the diagonal
    y = np.sin(3 * X[:, 0]) + 0.1 * rng.normal(size=n)
    logl = np.log(rng.uniform(0.3, 1.2, size=D if is_ard(kind) else 1))
    return X, y, logl


@pytest.mark.parametrize("kind", KINDS)
def test_closed_forms(kind):
    """n = 1: K_y = sigma^2 + noise + 1e-8, everything in closed form; k(x, x) = sigma^2 exactly; the D = 1 value against
    (1 + u^2 / (2 alpha l^2))^-alpha written with a power; symmetric to the bit."""
    ls, la, ln = 0.2, np.log(0.3), np.log(0.5)
    x = np.array([[0.3, 0.7]])
    logl = np.log([0.4, 0.9]) if is_ard(kind) else np.log([0.4])
    g = DenseGP(kind, dk.pack(kind, logl, ls, la, ln), x, [1.5], 0.5)
    c = np.exp(2 * ls) + np.exp(2 * ln) + 1e-8
    assert g.K[0, 0] == np.exp(2 * ls)
    assert abs(g.mll() - (-(1.0 / c + np.log(c) + np.log(2 * np.pi)) / 2)) <= 4 * EPS * abs(g.mll())
    ref = np.array([0.0] * logl.size + [0.0, (1.0 / c ** 2 - 1.0 / c) * np.exp(2 * ls), (1.0 / c ** 2 - 1.0 / c) * np.exp(2 * ln)])
    assert np.allclose(g.grad(), ref, rtol=1e-14, atol=1e-16)
    a = np.array([[0.0], [0.1]])
    b = np.array([[0.5], [0.1], [2.0]])
    K = dk.value(kind, dk.pack(kind, [np.log(0.4)], ls, la), a, b)
    ref = np.exp(2 * ls) * (1.0 + (a - b.T) ** 2 / (2 * 0.3 * 0.16)) ** -0.3
    assert np.allclose(K, ref, rtol=1e-14, atol=0) and K[1, 1] == np.exp(2 * ls)
    X, _, logl = _case(kind, 40, 3, 5)
    Ks = dk.value(kind, dk.pack(kind, logl, ls, la), X, X)
    assert np.array_equal(Ks, Ks.T) and np.all(np.diag(Ks) == np.exp(2 * ls))


def test_iso_is_ard_with_equal_lengthscales_to_the_bit():
    X, y, _ = _case(ISO_RQ, 50, 4, 6)
    a = DenseGP(ARD_RQ, dk.pack(ARD_RQ, np.full(4, np.log(0.6)), 0.1, 0.4, -1.0), X, y, 0.1)
    i = DenseGP(ISO_RQ, dk.pack(ISO_RQ, [np.log(0.6)], 0.1, 0.4, -1.0), X, y, 0.1)
    assert np.array_equal(a.K, i.K) and a.mll() == i.mll()
    ga, gi = a.grad(), i.grad()
    assert np.allclose(np.sum(ga[:4]), gi[0], rtol=1e-12) and np.array_equal(ga[4:], gi[1:])


@pytest.mark.parametrize("kind,alpha", [(k, a) for k in KINDS for a in (0.3, 2.0, 50.0)])
def test_dense_gradients_are_finite_at_duplicate_points_and_match_central_differences(kind, alpha):
    """Every component of grad (mll) and loo_grad (lpd), da included, against central differences of the restatement's own mll
    and LOO density; the input gradients against differences of its predictions, a test row on a training row included."""
    n, D = 60, 3
    X, y, logl = _case(kind, n, D, 7)
    h = np.concatenate([logl, [np.log(alpha), 0.1, np.log(0.3)]])

    def gp(v):
        return DenseGP(kind, v, X, y, 0.2)

    g0 = gp(h)
    ga, la = g0.grad(), g0.loo_grad()
    assert np.all(np.isfinite(ga)) and np.all(np.isfinite(la))
    step = 1e-5
    for j in range(h.size):
        hp, hm = h.copy(), h.copy()
        hp[j] += step
        hm[j] -= step
        p, m = gp(hp), gp(hm)
        for an, fd in ((ga[j], (p.mll() - m.mll()) / (2 * step)), (la[j], (p.loo()[2] - m.loo()[2]) / (2 * step))):
            assert abs(an - fd) <= 1e-6 * max(1.0, abs(fd)), (j, an, fd)
    Xt = np.vstack([X[4], np.random.default_rng(8).uniform(size=(5, D))])
    dmu, dvar = g0.input_gradients(Xt)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
    for d in range(D):
        Xp, Xm = Xt.copy(), Xt.copy()
        Xp[:, d] += step
        Xm[:, d] -= step
        (mp, vp), (mm, vm) = g0.prediction(Xp), g0.prediction(Xm)
        assert np.allclose((mp - mm) / (2 * step), dmu[:, d], rtol=1e-6, atol=1e-6)
        assert np.allclose((vp - vm) / (2 * step), dvar[:, d], rtol=1e-6, atol=1e-6)
    S = g0.prediction_cov(Xt)
    assert np.allclose(np.diag(S), g0.prediction(Xt)[1], rtol=1e-12, atol=1e-14)


def test_shape_derivative_is_nonpositive_and_quadratic_at_small_w():
    """dK/dlog alpha = k alpha (w / (1 + w) - log1p(w)) <= 0, and -k alpha w^2 / 2 to first order at small w."""
    X = np.array([[0.0], [1e-3], [0.5], [3.0]])
    g = DenseGP(ISO_RQ, dk.pack(ISO_RQ, [0.0], 0.0, np.log(2.0), -1.0), X, np.zeros(4), 0.0)
    dA = dk.d_hyper(ISO_RQ, g.h, X)[1][1]
    assert np.all(dA <= 0.0) and dA[0, 0] == 0.0
    w = dk.scaled_sqdist(ISO_RQ, g.h, X[:1], X[1:2])[0, 0] / (2.0 * 2.0)
    assert abs(dA[0, 1] - (-g.K[0, 1] * 2.0 * w * w / 2)) <= 2 * w * abs(dA[0, 1]) + EPS * g.K[0, 1] * 2.0 * w


def test_large_alpha_limit_is_the_squared_exponential():
    """With r^2 = sum u^2 / l^2: 0 <= k_RQ - k_SE <= k_SE (exp(r^4 / (8 alpha)) - 1), from w - w^2 / 2 <= log1p(w) <= w with
    alpha w = r^2 / 2, against the product-form SE at alpha = 1e6 (slack: a few roundings of either value)."""
    rng = np.random.default_rng(9)
    X = rng.uniform(size=(80, 3))
    logl, ls, alpha = np.log([0.4, 0.6, 0.9]), 0.1, 1e6
    Kr = dk.value(ARD_RQ, dk.pack(ARD_RQ, logl, ls, np.log(alpha)), X, X)
    r2 = np.sum((X[:, None, :] - X[None, :, :]) ** 2 / np.exp(2 * logl), axis=2)
    Ks = np.exp(2 * ls) * np.exp(-0.5 * r2)
    slack = Ks * (16 * EPS * (1.0 + r2))
    assert np.all(Kr - Ks >= -slack)
    assert np.all(Kr - Ks <= Ks * np.expm1(r2 * r2 / (8 * alpha)) + slack)
