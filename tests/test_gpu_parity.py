"""GPU suite: the HIP path, called through the C ABI (libdsmgp_hip.so), against the CPU oracle,
the committed golden vectors and size-independent properties.  Float64 throughout; tolerances are
stated per test (north star: predictive mean/variance within 1e-8 relative)."""
import json
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi, tree as ptree
from deepstructuredmixtures_amd.datagen import uniform, normal, regression_data
from oracle import gp as ogp, spn as ospn, scores as oscores

pytestmark = pytest.mark.gpu

RTOL = 1e-8   # north-star tolerance on predictive moments and log-marginals


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "gp_small.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    return cases


def _single(ctx, X, y, mean, kind, loghyp, logNoise):
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [mean])
    ctx.set_hyper(0, kind, np.concatenate([loghyp, [logNoise]]))
    return ctx.fit()


def test_native_library_is_loaded_and_sees_an_mi355x(ctx):
    assert os.path.exists(hipabi.LIB_PATH)
    name = ctx.device_name()
    assert "gfx950" in name, name


def test_mfma_f64_layout_exact_integers(ctx):
    """A = I / asymmetric-B style check of the f64 MFMA operand and result maps: with small integer
    data the blocked factorisation must reproduce an integer Cholesky factor EXACTLY."""
    n = 256
    rng = np.random.default_rng(5)
    Lt = np.tril(rng.integers(-3, 4, size=(n, n)).astype(np.float64), -1) + np.diag(rng.integers(1, 5, size=n).astype(float))
    A = Lt @ Lt.T          # exact in float64, asymmetric structure per tile
    # feed A through the IsoLinear kernel: K = X X^T / l^2 with X = Lt, l = 1, noise chosen to cancel eps
    X = Lt.copy()
    noise_var = 4.0
    ctx.set_train(X, np.zeros(n))
    ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
    ctx.set_hyper(0, 2, [0.0, 0.0, 0.5 * np.log(noise_var)])
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    F, _ = ctx.download_factor(0, n)
    ref = np.linalg.cholesky(A + (noise_var + 1e-8) * np.eye(n))
    assert np.max(np.abs(F - ref)) < 1e-11 * np.max(np.abs(ref))
    # rows/cols swapped inside a tile would give errors of order 1, not 1e-11


def test_kernel_matrix_against_oracle(ctx):
    D = 5
    x1 = uniform(50, 0, 300 * D).reshape((300, D), order="F")
    x2 = uniform(51, 0, 131 * D).reshape((131, D), order="F")
    ctx.set_train(x1, np.zeros(300))
    for kind, h in ((0, [np.log(0.4), 0.2]), (1, list(np.log([0.3, 0.5, 0.7, 0.9, 1.1])) + [-0.1]), (2, [np.log(1.7), 0.0])):
        ctx.set_hyper(0, kind, h + [0.0])
        K = ctx.kernel_matrix(0, x1, x2)
        Ko = ogp.kernelmatrix(ogp.make_kernel(kind, h), x1, x2, exact=True)
        assert np.max(np.abs(K - Ko)) <= 1e-13 * max(1.0, np.max(np.abs(Ko))), kind
        Kw = ogp.kernelmatrix(ogp.make_kernel(kind, h), x1, x2, exact=False)   # reference's GEMM-trick distances
        assert np.max(np.abs(K - Kw)) <= 1e-12 * max(1.0, np.max(np.abs(Ko))), kind


def test_golden_single_gps(ctx, golden_dir):
    """mpmath-pinned golden vectors: alpha, mll, predictive mean / variance, factor."""
    for name, c in _cases(golden_dir).items():
        n = c["X"].shape[0]
        mll, info, _ = _single(ctx, c["X"], c["y"], float(c["mean"]), int(c["kind"]), c["loghyp"], float(c["logNoise"]))
        assert info[0] == 0
        assert abs(mll[0] - float(c["mll"])) <= RTOL * max(1.0, abs(float(c["mll"]))), name
        F, alpha = ctx.download_factor(0, n)
        assert np.max(np.abs(F - c["L"])) <= 1e-11 * np.max(np.abs(c["L"])), name
        assert np.allclose(alpha, c["alpha"], rtol=1e-8, atol=1e-10), name
        nt = c["Xt"].shape[0]
        mu, var = ctx.predict_leaves(c["Xt"], [0, nt], np.arange(nt))
        assert np.allclose(mu, c["mu"], rtol=RTOL, atol=1e-11), name
        assert np.allclose(var, c["var"], rtol=RTOL, atol=1e-11), name


def test_analytic_closed_forms(ctx, golden_dir):
    a = json.load(open(os.path.join(golden_dir, "analytic.json")))
    for name in ("n1", "n2"):
        c = a[name]
        X = np.atleast_1d(np.array(c["x"], dtype=float)).reshape(-1, 1)
        y = np.atleast_1d(np.array(c["y"], dtype=float))
        mll, info, _ = _single(ctx, X, y, c["mean"], 0, np.array([c["logl"], c["logs"]]), c["logNoise"])
        assert abs(mll[0] - c["mll"]) < 1e-12 * max(1, abs(c["mll"]))
        mu, var = ctx.predict_leaves(np.array([[c["xt"]]]), [0, 1], [0])
        assert abs(mu[0] - c["mu"]) < 1e-13 and abs(var[0] - c["var"]) < 1e-13


@pytest.mark.parametrize("n,D,kind", [(127, 1, 0), (128, 2, 0), (129, 3, 0), (700, 4, 0), (1000, 8, 1), (515, 3, 2),
                                       (2500, 8, 0)])
def test_single_gp_vs_oracle(ctx, n, D, kind):
    """Config-2 shape at oracle-sized n, ragged sizes around the 128 tile edge, every kernel kind."""
    X = uniform(60 + n, 0, n * D).reshape((n, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.1 * normal(61 + n, 0, n)
    Xt = uniform(62 + n, 0, 150 * D).reshape((150, D), order="F")
    h = {0: [np.log(0.3), 0.0], 1: list(np.log(np.linspace(0.3, 0.8, D))) + [0.1], 2: [np.log(0.9), 0.0]}[kind]
    logNoise = np.log(0.1)
    mean = float(np.mean(y))
    mll, info, _ = _single(ctx, X, y, mean, kind, np.array(h), logNoise)
    g = ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, h), logNoise, exact_dist=True).update_cholesky()
    assert info[0] == 0 and g.info == 0
    assert abs(mll[0] - g.mll()) <= RTOL * max(1.0, abs(g.mll()))
    F, alpha = ctx.download_factor(0, n)
    assert np.max(np.abs(F - g.L())) <= 1e-9 * np.max(np.abs(g.L()))
    assert np.max(np.abs(alpha - g.alpha)) <= 1e-7 * np.max(np.abs(g.alpha))
    mu, var = ctx.predict_leaves(Xt, [0, 150], np.arange(150))
    mo, vo = g.prediction(Xt)
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9)
    assert np.allclose(var, vo, rtol=RTOL, atol=1e-10)


@pytest.mark.parametrize("n,D,logl,lognoise", [(128, 2, np.log(0.3), np.log(0.1)), (777, 3, np.log(0.5), np.log(0.01)),
                                               (2000, 2, np.log(0.8), np.log(0.003))])
def test_cholesky_backward_error(ctx, n, D, logl, lognoise):
    """||K_y - L L^T||_F <= a few ulps of ||K_y||_F with K_y from the device's own Gram kernel: only the factorisation
    (the 16x16 diagonal blocks eliminated four pivots at a time with an explicitly inverted 4x4 factor and rank-4 MFMA
    updates, MFMA trailing updates, split-K) is measured; cond(K_y) up to 1e8."""
    rng = np.random.default_rng(n)
    X = np.asfortranarray(rng.random((n, D)))
    ctx.set_train(X, rng.standard_normal(n))
    ctx.set_leaves(np.array([0, n]), np.arange(n), [0], [0.0])
    ctx.set_sharing(None, None, None)
    ctx.set_hyper(0, 0, [logl, 0.0, lognoise])
    _, info, _ = ctx.fit()
    assert info[0] == 0
    F, _ = ctx.download_factor(0, n)
    L = np.tril(F)
    K = ctx.kernel_matrix(0, X, X) + (np.exp(2 * lognoise) + 1e-8) * np.eye(n)
    assert np.linalg.norm(K - L @ L.T) <= 4e-15 * np.linalg.norm(K)


def test_not_positive_definite_is_reported(ctx):
    """LAPACK-style info: a rank-1 linear-kernel Gram of size 1e16 leaves only rounding noise (+-1) in the
    Schur complement, far above noise + eps, so some pivot goes non-positive -- in LAPACK and here."""
    import scipy.linalg as sla
    n = 140
    X = np.linspace(1.0, 2.0, n).reshape(-1, 1) * 1e8
    ctx.set_train(X, np.zeros(n))
    ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    _, info, _ = ctx.fit()
    K = X @ X.T + (np.exp(-60.0) + 1e-8) * np.eye(n)
    _, linfo = sla.lapack.dpotrf(K, lower=1)
    assert linfo > 0 and 1 < info[0] <= n


def test_first_bad_minor_is_reported_exactly(ctx):
    """Deterministic non-positive-definite cases with a KNOWN first bad leading minor: IsoLinear kernel
    (K = X X^T / l^2, l = 1) on rows 2^27 e_i, so K = 2^54 x (0/1 matrix) and noise + eps (< 1) is absorbed by rounding
    (ulp(2^54) = 4): every operation of the factorisation is exact in binary floating point -- sqrt(2^54) = 2^27,
    1 / 2^54 -- and a repeated row makes its pivot exactly 0.  `info` must EQUAL LAPACK's: the index of that row
    (1-based), inside the first 128-block and, with D = 131 orthogonal directions, at row 131 of the second block (the
    blocked path: panel solve, update of the next diagonal tile, global row offset of the block)."""
    import scipy.linalg as sla
    # the two cases of round 3's first version, then one case per place a pivot can sit in since the diagonal 16x16 blocks
    # are eliminated four pivots at a time on the matrix pipe: every position inside a group of four, first and last group of
    # a 16x16 block, first / inner / last 16x16 block of a tile, first and second row of the second and third tile
    cases = [(3, 140, 3), (131, 140, 130)] + [(rep + 1, 300, rep) for rep in (1, 2, 4, 5, 6, 7, 12, 15, 16, 19, 47, 62, 64, 111,
                                                                               126, 127, 128, 129, 143, 200, 255, 256, 257, 299)]
    for D, n, rep in cases:
        X = np.zeros((n, D))
        for i in range(min(n, D)):
            X[i, i] = 2.0 ** 27
        X[rep, :] = 0.0
        X[rep, 0] = 2.0 ** 27                                        # row `rep` repeats row 0: the first dependent row
        for i in range(rep + 1, n):
            X[i, :] = 0.0
            X[i, (i * 7) % D] = 2.0 ** 27                            # what follows the bad pivot does not matter
        ctx.set_train(X, np.zeros(n))
        ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
        ctx.set_sharing(None, None, None)
        ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
        _, info, _ = ctx.fit()
        K = X @ X.T + (np.exp(-60.0) + 1e-8) * np.eye(n)
        assert K[rep, rep] == 2.0 ** 54                              # the shift is absorbed
        _, linfo = sla.lapack.dpotrf(K, lower=1)
        assert linfo == rep + 1 and info[0] == linfo, (D, int(info[0]), linfo)


def test_error_paths(ctx):
    with pytest.raises(hipabi.DsmgpError):
        ctx.set_leaves([0, 3], [2, 1, 0], [0], [0.0])               # not ascending
    X = uniform(1, 0, 40).reshape((20, 2), order="F")
    ctx.set_train(X, np.zeros(20))
    ctx.set_leaves([0, 10, 20], np.arange(20), [0, 1], [0.0, 0.0])
    ctx.set_hyper(0, 0, [0.0, 0.0, 0.0])
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.fit()                                                    # kernel id 1 has no hyper-parameters
    assert "kernel id 1" in str(e.value)
    with pytest.raises(hipabi.DsmgpError):
        ctx.set_sharing([0, 1], [-1, 0], [0, 0])                     # COPY claim with different obs lists
    with pytest.raises(hipabi.DsmgpError):
        ctx.set_hyper(0, 1, [0.0, 0.0, 0.0])                         # ArdSE needs D lengthscales
        ctx.set_hyper(1, 0, [0.0, 0.0, 0.0])
        ctx.fit()


def _oracle_model(m, X, y, tau=0.05):
    gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
    census = ospn.fit(m.root, gps, ospn.get_overlap(m.root, m.L), tau)
    return gps, census


def test_config1_readme_example(golden_dir):
    """BASELINE config 1 (README 1-D sinusoid, N=100, IsoSE(1,1), K=4, V=3, M=10): every sharing branch
    fires here (copy, prefix continue); compared with the committed oracle fixture."""
    z = np.load(os.path.join(golden_dir, "config1.npz"))
    X, y, xt = z["x"].reshape(-1, 1), z["y"], z["xt"]
    m = dsm.buildDSMGP(X, y, 3, 4, M=10, kernel=dsm.IsoSE(1.0, 1.0), meanFun=dsm.ConstMean(float(np.mean(X))), seed=11)
    assert np.count_nonzero(m.share_op == ptree.SHARE_COPY) == z["census"][1] > 0
    assert np.count_nonzero(m.share_op == ptree.SHARE_PREFIX) == z["census"][2] > 0
    # the census of the reference's fit! arms rides on fit's return value and stays on the model: equal to the fixture
    # (generated by the oracle's fit) and to the oracle's census walk
    assert [m.fit_census[k] for k in ptree.BRANCH_NAMES] == z["census"].tolist()
    assert m.fit_census == ospn.fit(m.root, None, ospn.get_overlap(m.root, m.L), 0.05, census_only=True)
    assert m.fit_census["lowrank_leaves"] == [] and len(m.fit_census["leading_leaves"]) == z["census"][4] > 0
    assert dsm.fit(m, tau=0.5).census["lowrank_as_full"] > 0          # with a generous tau the row-deletion arm would fire
    dsm.fit(m)
    assert np.allclose(m.leaf_mll, z["leaf_mll"], rtol=RTOL, atol=1e-9)
    zroot = dsm.update(m)
    assert abs(zroot - float(z["root_mll"])) <= RTOL * abs(float(z["root_mll"]))
    mu, var = dsm.predict(m, xt)
    assert np.allclose(mu, z["mu"], rtol=RTOL, atol=1e-10)
    assert np.allclose(var, z["var"], rtol=RTOL, atol=1e-10)
    # fit_naive! (no sharing) gives the same model
    dsm.fit_naive(m)
    assert np.allclose(m.leaf_mll, z["leaf_mll"], rtol=RTOL, atol=1e-9)


def test_resident_test_rows_riding_through_fit_equal_the_standalone_predict():
    """With a test set resident, fit advances K_tn L^-T inside the factorisation launches and predict only
    finishes mu/var; without it predict runs its own sweep.  Same numbers either way (summation order of the
    split-K pieces may differ: 1e-11), for DSMGP (routed rows) and PoE (all rows to all leaves), incl. COPY leaves."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "config1.npz"))
    X1, y1, xt1 = z["x"].reshape(-1, 1), z["y"], z["xt"]
    X, y, Xt = regression_data(5000, 4, n_test=700, seed=1234)
    cases = [lambda: dsm.buildDSMGP(X, y, 3, 4, M=100, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=8),
             lambda: dsm.buildPoE(X, y, 4, M=300, kernel=dsm.ArdSE(np.log([0.3, 0.4, 0.5, 0.6]), 0.0), logNoise=np.log(0.2),
                                  meanFun=dsm.ConstMean(0.1), seed=8),
             lambda: dsm.buildDSMGP(X1, y1, 3, 4, M=10, kernel=dsm.IsoSE(1.0, 1.0), meanFun=dsm.ConstMean(0.5), seed=11)]
    for make, xt in zip(cases, (Xt, Xt, xt1)):
        m = make()
        m.ctx.set_profile(True)                   # per-category device times
        mu0, v0 = dsm.predict(m, xt)              # standalone sweep (fit ran before the test set existed)
        t = m.ctx.timings()
        assert t["predict_update"] + t["predict_trsm"] > 0     # a sweep of its own (fused steps: no panel-solve launches)
        dsm.fit(m)                                # test rows ride along
        mu1, v1 = dsm.predict(m, xt)
        t = m.ctx.timings()
        assert t["predict_update"] == 0.0 and t["predict_trsm"] == 0.0
        assert np.allclose(mu1, mu0, rtol=1e-11, atol=1e-12) and np.allclose(v1, v0, rtol=1e-10, atol=1e-13)
        m.ctx.set_joint(False)
        dsm.fit(m)
        mu2, v2 = dsm.predict(m, xt)
        assert np.array_equal(mu2, mu0) and np.array_equal(v2, v0)   # same path as the first time: same bits
        m.ctx.set_joint(True)
    # a test set announced before the very first fit rides along from the start
    m3 = dsm.buildDSMGP(X, y, 3, 4, M=100, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=8, fit_now=False)
    dsm.resident_test(m3, Xt)
    m3.ctx.set_profile(True)
    dsm.fit(m3)
    mu3, v3 = dsm.predict(m3, Xt)
    t = m3.ctx.timings()
    assert t["predict_update"] == 0.0 and t["predict_trsm"] == 0.0
    mref, vref = dsm.predict(cases[0](), Xt)
    assert np.allclose(mu3, mref, rtol=1e-11, atol=1e-12) and np.allclose(v3, vref, rtol=1e-10, atol=1e-13)


def test_prefix_continue_equals_full_factorisation(ctx):
    """chol_continue! property (src/AdvancedCholeskey.jl:121-135's intent): continuing from a copied
    leading block == factorising from scratch, at sizes that cross several 128-blocks."""
    N, D = 900, 2
    X = uniform(70, 0, N * D).reshape((N, D), order="F")
    y = np.cos(3 * X[:, 0]) + 0.05 * normal(71, 0, N)
    p = 400                                     # 3 whole blocks copied, block 3 recomputed
    obs_ptr = [0, p, p + N]
    obs_idx = np.concatenate([np.arange(p), np.arange(N)])
    ctx.set_train(X, y)
    ctx.set_leaves(obs_ptr, obs_idx, [0, 0], [0.1, 0.2])
    ctx.set_hyper(0, 0, [np.log(0.3), 0.0, np.log(0.1)])
    ctx.set_sharing([0, 2], [-1, 0], [0, p])
    mll_s, info, _ = ctx.fit()
    F_s, a_s = ctx.download_factor(1, N)
    ctx.set_sharing(None, None, None)
    mll_f, info2, _ = ctx.fit()
    F_f, a_f = ctx.download_factor(1, N)
    assert info[1] == 0 and info2[1] == 0
    assert np.max(np.abs(F_s - F_f)) <= 1e-12 * np.max(np.abs(F_f))
    assert np.allclose(mll_s, mll_f, rtol=1e-12)
    assert np.allclose(a_s, a_f, rtol=1e-9, atol=1e-11)
    g = ogp.GaussianProcess(X, y, 0.2, ogp.IsoSE(np.log(0.3), 0.0), np.log(0.1), True).update_cholesky()
    assert abs(mll_s[1] - g.mll()) <= RTOL * abs(g.mll())


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gpoe", "rbcm", "kernel_vector", "ardse"])
def test_models_vs_oracle(family):
    """Whole models at oracle size: leaf log-marginals, update!, predict for every model family."""
    N, D = 3000, 3
    X, y, Xt = regression_data(N, D, n_test=200, seed=900)
    kern = dsm.IsoSE(np.log(0.3), 0.0)
    kw = dict(logNoise=np.log(0.1), seed=4)
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 3, 4, M=60, kernel=kern, **kw)
    elif family == "kernel_vector":
        m = dsm.buildDSMGP(X, y, 2, 4, M=60, kernel=[kern, dsm.IsoLinear(np.log(1.5))], **kw)
    elif family == "ardse":
        m = dsm.buildDSMGP(X, y, 2, 4, M=60, kernel=dsm.ArdSE(np.log([0.3, 0.4, 0.5]), 0.0), **kw)
    elif family == "poe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), **kw)
    elif family == "gpoe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), generalized=True, **kw)
    else:
        m = dsm.buildBCM(X, y, 8, M=100, kernel=kern, **kw)
    gps, _ = _oracle_model(m, X, y)
    lo = np.array([g.mll() for g in gps])
    assert np.allclose(m.leaf_mll, lo, rtol=RTOL, atol=1e-8)
    if m.family == "dsmgp":
        z = dsm.update(m)
        zo = ospn.update(m.root, gps)
        assert abs(z - zo) <= RTOL * max(1.0, abs(zo))
        mo, vo = ospn.predict(m.root, gps, Xt)
    elif m.family == "poe":
        mo, vo = ospn.predict_poe(m.root, gps, Xt)
    elif m.family == "gpoe":
        mo, vo = ospn.predict_gpoe(m.root, gps, Xt)
    else:
        mo, vo = ospn.predict_rbcm(m.root, gps, Xt)
    mu, var = dsm.predict(m, Xt)
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9), float(np.max(np.abs(mu - mo)))
    assert np.allclose(var, vo, rtol=RTOL, atol=1e-10), float(np.max(np.abs(var - vo) / vo))


def test_depth4_many_small_leaves_vs_oracle():
    """The small-M panel regime of SURVEY 8(a) (config 4'': depth 4, thousands of leaves of a few blocks at most):
    more than 8192 leaves, so the overlap matrix stays sparse (tree.LeafOverlap) and update!/predict run their
    level-order passes; leaf log-marginals, the sharing census, update! and predict against the oracle."""
    N, D = 12000, 3
    X, y, Xt = regression_data(N, D, n_test=300, seed=77)
    m = dsm.buildDSMGP(X, y, 2, 5, M=8, D=4, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=9)
    assert m.L > 8192 and isinstance(m.D, ptree.LeafOverlap)
    gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
    census = ospn.fit(m.root, gps, m.D.todense(), 0.05)
    assert np.count_nonzero(m.share_op == ptree.SHARE_COPY) == census["copy"] > 0
    assert np.count_nonzero(m.share_op == ptree.SHARE_PREFIX) == census["prefix"] > 0
    lo = np.array([g.mll() for g in gps])
    assert np.allclose(m.leaf_mll, lo, rtol=RTOL, atol=1e-8)
    z, zo = dsm.update(m), ospn.update(m.root, gps)
    assert abs(z - zo) <= RTOL * max(1.0, abs(zo))
    mo, vo = ospn.predict(m.root, gps, Xt)
    mu, var = dsm.predict(m, Xt)
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9), float(np.max(np.abs(mu - mo)))
    assert np.allclose(var, vo, rtol=RTOL, atol=1e-10), float(np.max(np.abs(var - vo) / vo))


@pytest.mark.parametrize("kind,n,D", [(0, 300, 2), (0, 1111, 5), (1, 400, 3), (2, 333, 2)])
def test_gradients_vs_oracle(ctx, kind, n, D):
    """updategradients!(gp): [dl..., ds, dnoise] with the reference's scaling and ArdSE dl == 0 (F6)."""
    X = uniform(80 + n, 0, n * D).reshape((n, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.1 * normal(81 + n, 0, n)
    h = {0: [np.log(0.4), 0.2], 1: list(np.log(np.linspace(0.4, 0.9, D))) + [-0.1], 2: [np.log(0.9), 0.0]}[kind]
    ln = np.log(0.25)
    mean = float(np.mean(y))
    _single(ctx, X, y, mean, kind, np.array(h), ln)
    g = ctx.gradients(len(h) + 1)[0]
    go = ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, h), ln, True).update_cholesky().grad()
    scale = max(1.0, float(np.max(np.abs(go))))
    assert np.max(np.abs(g - go)) <= 1e-7 * scale, (g, go)
    if kind == 1:
        assert np.all(g[:D] == 0.0)


def test_train_loop_follows_the_oracle_trajectory():
    """train! (src/optimisers.jl:4-87) for a few iterations: same mll history and hyper-parameters as the
    oracle-driven loop (gradient ascent, stateless ADAM step)."""
    N, D = 1500, 2
    X, y, _ = regression_data(N, D, n_test=10, seed=321)
    m = dsm.buildDSMGP(X, y, 2, 4, M=60, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.3), seed=9)
    _, hist = dsm.train(m, dsm.ADAM(eta=0.02), iterations=4, randinit=False)
    trained = dsm.getparams(m).copy()
    hyp = np.array([np.log(0.5), 0.0, np.log(0.3)])
    ref = []
    opt = dsm.ADAM(eta=0.02)
    for it in range(4):
        dsm.setparams(m, hyp)
        gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
        ospn.fit_naive(m.root, gps)
        ref.append(ospn.mll(m.root, gps))
        hyp = hyp + opt.apply(hyp, ospn.grad_tree(m.root, gps, 3))
    assert np.allclose(hist, ref, rtol=1e-8)
    assert np.allclose(trained, hyp, rtol=1e-9, atol=1e-12)
    assert hist[-1] > hist[0]


def test_gradient_leaf_mask_computes_only_what_is_asked_for(ctx):
    """dsmgp_set_gradient_leaves: the rows of the active leaves equal the unmasked gradients (to rounding: with
    fewer tiles in a launch the K ranges are cut differently, so sums change order in the last bits), the others are zero,
    and the pass does proportionally less -- also for an active COPY leaf whose source is inactive (its
    source's contraction and factor are pulled in) and for an active PREFIX leaf."""
    N, D, L = 6000, 3, 6
    X, y, _ = regression_data(N, D, n_test=10, seed=915)
    rng = np.random.default_rng(5)
    sizes = [700, 900, 1300, 500, 900, 800]
    obs = [np.sort(rng.choice(N, size=n, replace=False)) for n in sizes]
    obs[4] = obs[1].copy()                                                  # COPY of leaf 1
    tail = np.arange(obs[3][-1] + 1, min(N, obs[3][-1] + 301))
    obs[5] = np.concatenate([obs[3], tail])                                 # leaf 3 is a prefix of leaf 5
    op = np.array([0, 0, 0, 0, 1, 2], dtype=np.int32)
    src = np.array([-1, -1, -1, -1, 1, 3], dtype=np.int32)
    plen = np.array([0, 0, 0, 0, 0, obs[3].size], dtype=np.int64)
    means = [float(np.mean(y[o])) for o in obs]
    means[4] = means[1]
    ctx.set_train(X, y)
    ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, dtype=np.int32), means)
    ctx.set_sharing(op, src, plen)
    ctx.set_hyper(0, 0, [np.log(0.3), 0.1, np.log(0.2)])
    ctx.fit()
    full = ctx.gradients(3)
    t_full = ctx.timings()["gradients"]
    assert np.all(full != 0)
    for active in ([0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1], [1, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0]):
        ctx.set_gradient_leaves(active)
        g = ctx.gradients(3)
        a = np.array(active, dtype=bool)
        assert np.allclose(g[a], full[a], rtol=1e-11, atol=0) and np.all(g[~a] == 0)
    ctx.set_gradient_leaves([0, 0, 0, 1, 0, 0])                             # the smallest leaf alone: a fraction of the pass
    ctx.gradients(3)
    assert ctx.timings()["gradients"] < 0.6 * t_full
    ctx.set_gradient_leaves(None)
    assert np.array_equal(ctx.gradients(3), full)


def test_finetune_follows_the_oracle_loop():
    """finetune! (src/finetuning.jl:8-87): L whole-tree fit! + updategradients! passes per iteration on the device,
    per-leaf hyper-vectors at the end (a kernel id per leaf); same history and vectors as the oracle's loop."""
    X, y, Xt = regression_data(900, 2, n_test=50, seed=77)
    kw = dict(M=60, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.3), seed=6)
    m = dsm.buildDSMGP(X, y, 2, 3, **kw)
    ref = dsm.buildDSMGP(X, y, 2, 3, fit_now=False, **kw)
    _, hist = dsm.finetune(m, dsm.ADAM(eta=0.03), iterations=2)
    gps = ospn.make_leaf_gps(ref.root, X, y, exact_dist=True)
    hyp, hist_ref = ospn.finetune(ref.root, gps, ospn.get_overlap(ref.root, ref.L), dsm.ADAM(eta=0.03).apply, 2)
    assert np.allclose(hist, hist_ref, rtol=1e-8)
    got = np.array([np.concatenate([lf.kernel.loghyp(), [lf.logNoise]]) for lf in m.leaves])
    assert np.allclose(got, np.array(hyp), rtol=1e-7, atol=1e-10)
    assert np.allclose(m.leaf_mll, [g.mll() for g in gps], rtol=RTOL, atol=1e-8)
    # the model with per-leaf hyper-parameters still predicts (leaves now carry kernel ids of their own)
    for lf, hv in zip(ref.leaves, hyp):
        lf.kernel.set_loghyp(hv[:-1])
        lf.logNoise = float(hv[-1])
    dsm.update(m)
    mu, var = dsm.predict(m, Xt)
    ospn.update(ref.root, gps)
    mo, vo = ospn.predict(ref.root, gps, Xt)
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9) and np.allclose(var, vo, rtol=RTOL, atol=1e-10)


def test_full_size_properties_single_large_gp(ctx):
    """Config 2 (single exact GP N=4096, D=4, IsoSE) -- too large to compare entry by entry quickly,
    checked through size-independent properties: L L^T = K, K alpha = y, mll consistency,
    predictions at training points, refit idempotence."""
    N, D = 4096, 4
    X, y, Xt = regression_data(N, D, n_test=256, seed=20202)
    h = np.array([np.log(0.3), 0.0])
    ln = np.log(0.1)
    mean = float(np.mean(y))
    mll, info, sec = _single(ctx, X, y, mean, 0, h, ln)
    assert info[0] == 0
    F, alpha = ctx.download_factor(0, N)
    K = ogp.kernelmatrix(ogp.IsoSE(*h), X, None, exact=True)
    K[np.diag_indices(N)] += np.exp(2 * ln) + 1e-8
    assert np.max(np.abs(F @ F.T - K)) <= 1e-12 * N
    yc = y - mean
    assert np.max(np.abs(K @ alpha - yc)) <= 1e-8 * np.max(np.abs(yc))
    mll_host = -(yc @ alpha + 2 * np.sum(np.log(np.diag(F))) + N * np.log(2 * np.pi)) / 2
    assert abs(mll[0] - mll_host) <= 1e-10 * abs(mll_host)
    # predicting at training inputs: mu = y - noise*alpha  (K_f alpha = yc - (noise+eps) alpha)
    idx = np.arange(0, N, 16)
    mu, var = ctx.predict_leaves(X[idx], [0, idx.size], np.arange(idx.size))
    assert np.allclose(mu, y[idx] - (np.exp(2 * ln) + 1e-8) * alpha[idx], rtol=1e-9, atol=1e-10)
    assert np.all(var > np.exp(2 * ln)) and np.all(var < 1.0 + np.exp(2 * ln) + 1e-12)
    mll2, _, _ = ctx.fit()
    assert mll2[0] == mll[0]                                         # deterministic, idempotent
    g_mu, g_var = ctx.predict_leaves(Xt, [0, 256], np.arange(256))
    go = ogp.GaussianProcess(X, y, mean, ogp.IsoSE(*h), ln, True).update_cholesky()
    mo, vo = go.prediction(Xt)
    assert abs(mll[0] - go.mll()) <= RTOL * abs(go.mll())
    assert np.allclose(g_mu, mo, rtol=RTOL, atol=1e-9) and np.allclose(g_var, vo, rtol=RTOL, atol=1e-10)


_SHARD_WORKER = r"""
import os, sys
import numpy as np
import torch.distributed as td
sys.path.insert(0, {root!r})
import deepstructuredmixtures_amd as dsm
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
td.init_process_group("gloo", rank=rank, world_size=world)
X, y, Xt = dsm.regression_data(4000, 3, n_test=300, seed=77)
ref = np.load({ref!r})
m = dsm.buildDSMGP(X, y, 3, 4, M=80, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=5,
                   shard_world=(rank, world))
assert 0 < len(m.shard.local) < m.L
z = dsm.update(m)
mu, var = dsm.predict(m, Xt)
# per-leaf values: to rounding, not to the bit -- how a block step is scheduled (fused or classic launches, how many K-pieces
# per tile) depends on how many leaves and tiles share the launch, i.e. on the shard
assert np.allclose(m.leaf_mll, ref["leaf_mll"], rtol=1e-12, atol=0) and abs(z - float(ref["z"])) <= 1e-12 * abs(float(ref["z"]))
# predict: every rank aggregates its own leaves on its device, the partial sums are added in rank order -- another
# association than the single-context sum over all leaves, the same terms
assert np.allclose(mu, ref["mu"], rtol=1e-12, atol=1e-13) and np.allclose(var, ref["var"], rtol=1e-10, atol=1e-13)
dsm.updategradients(m)
assert np.allclose(dsm.grad_mll(m), ref["grad"], rtol=1e-9, atol=1e-9)
both = [None, None]
td.all_gather_object(both, (m.leaf_mll.tobytes(), mu.tobytes(), var.tobytes()))
assert both[0] == both[1]                       # the ranks hold the same bits
td.barrier(); td.destroy_process_group()
print("rank", rank, "ok", len(m.shard.local))
"""


def test_two_ranks_sharing_leaves_reproduce_the_single_process_result(tmp_path):
    """Leaf sharding through the real HIP contexts (two processes on the one GPU of this box, gloo for the
    all-gathers): per-leaf results (log-marginals, gradients) equal the unsharded run's to rounding (1e-12: the launch
    schedule of a block step depends on how many leaves share it), the aggregated prediction adds per-rank partial sums and
    agrees to rounding, and both ranks end up with the SAME bits."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    X, y, Xt = regression_data(4000, 3, n_test=300, seed=77)
    m = dsm.buildDSMGP(X, y, 3, 4, M=80, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=5)
    z = dsm.update(m)
    mu, var = dsm.predict(m, Xt)
    dsm.updategradients(m)
    ref = str(tmp_path / "ref.npz")
    np.savez(ref, leaf_mll=m.leaf_mll, z=z, mu=mu, var=var, grad=dsm.grad_mll(m))
    script = tmp_path / "worker.py"
    script.write_text(_SHARD_WORKER.format(root=root, ref=ref))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29000 + os.getpid() % 2000), WORLD_SIZE="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-2000:]


def test_config3_poe_ardse_full_size_sampled_against_oracle():
    """BASELINE config 3 at full size: buildPoE K=8 splits, M=200, N=50k, D=8, additive ArdSE.  Every leaf is
    oracle-sized (n ~ 200-400), so a sample of leaves is compared entry-wise and the PoE rule on top of them."""
    N, D = 50_000, 8
    X, y, Xt = regression_data(N, D, n_test=64, seed=20203)
    kern = dsm.ArdSE(np.log(np.full(D, 0.3)), 0.0)
    m = dsm.buildPoE(X, y, 8, M=200, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), logNoise=np.log(0.1), seed=3)
    assert m.L >= 100 and max(lf.nobs for lf in m.leaves) <= 401
    gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
    sample = list(range(0, m.L, max(1, m.L // 12)))
    for j in sample:
        gps[j].update_cholesky()
        assert abs(m.leaf_mll[j] - gps[j].mll()) <= RTOL * abs(gps[j].mll())
    ptr = np.arange(m.L + 1) * Xt.shape[0]
    mu_l, var_l = m.ctx.predict_leaves(Xt, ptr, np.tile(np.arange(Xt.shape[0]), m.L))
    for j in sample:
        mo, vo = gps[j].prediction(Xt)
        assert np.allclose(mu_l[ptr[j]:ptr[j + 1]], mo, rtol=RTOL, atol=1e-9)
        assert np.allclose(var_l[ptr[j]:ptr[j + 1]], vo, rtol=RTOL, atol=1e-10)
    mu, var = dsm.predict(m, Xt)
    t = 1.0 / var_l.reshape(m.L, -1)
    assert np.allclose(var, 1.0 / t.sum(0), rtol=1e-12)
    assert np.allclose(mu, (t * mu_l.reshape(m.L, -1)).sum(0) / t.sum(0), rtol=1e-11, atol=1e-12)


def test_config4_headline_size_sampled_against_oracle_and_properties():
    """BASELINE config 4 (the bench workload): buildDSMGP K=4 splits V=3 M=200 N=100k D=8 IsoSE, 144 leaves with
    n ~ 1.4k-13k.  Too large for a full oracle run: three sampled leaves are compared with the oracle (mll,
    alpha, predictions), and the whole model through size-independent properties."""
    import bench
    model, X, y, Xt, ptr, idx = bench.build_model("dsmgp_n100k_d8", 0, 1, 0)
    assert model.L == 144
    sec = dsm.fit(model)
    # census of the reference's fit! arms, surfaced by fit (index work: exact): the oracle's walk over the same decisions
    # gives the same counts and the same leaves for the arms this implementation computes in full
    cen = ospn.fit(model.root, None, model.D, 0.05, census_only=True)
    assert sec.census == model.fit_census == cen and sum(cen[k] for k in ptree.BRANCH_NAMES) == 144
    assert np.count_nonzero(model.share_op == ptree.SHARE_COPY) == cen["copy"]
    assert np.count_nonzero(model.share_op == ptree.SHARE_PREFIX) <= cen["prefix"]     # a PREFIX source must be factorised in full
    z = dsm.update(model)
    mu, var = dsm.predict(model, Xt)
    nobs = np.array([lf.nobs for lf in model.leaves])
    order = np.argsort(nobs)
    mu_l, var_l = model.ctx.predict_fetch()
    for j in (order[0], order[20], order[60]):              # n = 1.4k, ~3k, ~5k
        lf = model.leaves[j]
        g = ogp.GaussianProcess(X[lf.obs], y[lf.obs], lf.mean.m, ogp.IsoSE(lf.kernel.logl, lf.kernel.logs), lf.logNoise,
                                exact_dist=True).update_cholesky()
        assert abs(model.leaf_mll[j] - g.mll()) <= RTOL * abs(g.mll())
        _, alpha = model.ctx.download_factor(j, lf.nobs)
        assert np.max(np.abs(alpha - g.alpha)) <= 1e-7 * np.max(np.abs(g.alpha))
        rows = idx[ptr[j]:ptr[j + 1]]
        mo, vo = g.prediction(Xt[rows])
        assert np.allclose(mu_l[ptr[j]:ptr[j + 1]], mo, rtol=RTOL, atol=1e-9)
        assert np.allclose(var_l[ptr[j]:ptr[j + 1]], vo, rtol=RTOL, atol=1e-10)
    # The leaves that matter: the largest one (n ~ 13k: most block steps, deepest split-K, worst
    # conditioning, on the multi-GPU critical path) and one of ~9k rows, against the oracle entry by entry, plus the
    # backward error of the downloaded factor  ||K_y - L L^T||_F <= 1e-14 ||K_y||_F  and the residual of K_y alpha = y.
    import scipy.linalg as sla
    big = [int(order[-1]), int(order[np.searchsorted(nobs[order], 9000)])]
    assert nobs[big[0]] > 13000 and 8500 < nobs[big[1]] < 10500
    for j in big:
        lf = model.leaves[j]
        g = ogp.GaussianProcess(X[lf.obs], y[lf.obs], lf.mean.m, ogp.IsoSE(lf.kernel.logl, lf.kernel.logs), lf.logNoise,
                                exact_dist=True)
        Ky = g.noisy_kernel()
        g.P = None                                       # 1.4 GB at n = 13k: not needed again
        C, info = sla.lapack.dpotrf(Ky, lower=1, clean=1)
        g.factors, g.info = C, int(info)
        g.solve_alpha()
        assert info == 0 and abs(model.leaf_mll[j] - g.mll()) <= RTOL * abs(g.mll())
        F, alpha = model.ctx.download_factor(j, lf.nobs)
        assert np.max(np.abs(alpha - g.alpha)) <= 1e-7 * np.max(np.abs(g.alpha))
        assert np.max(np.abs(F - C)) <= 1e-9 * np.max(np.abs(C))
        yc = y[lf.obs] - lf.mean.m
        assert np.max(np.abs(Ky @ alpha - yc)) <= 1e-8 * np.max(np.abs(yc))
        R = sla.blas.dsyrk(1.0, F, lower=1)              # lower triangle of L L^T
        R -= np.tril(Ky)
        off = np.tril(R, -1)
        res = np.sqrt(2.0 * np.sum(off * off) + np.sum(np.diag(R) ** 2))
        assert res <= 1e-14 * np.linalg.norm(Ky), (lf.nobs, res / np.linalg.norm(Ky))
        del R, off, F, Ky
        rows = idx[ptr[j]:ptr[j + 1]]
        Knt = ogp.kernelmatrix(g.kernel, g.x, Xt[rows], True)
        mo = g.mean + Knt.T @ g.alpha
        V = sla.solve_triangular(C, Knt, lower=True)
        vo = ogp.prior_diag(g.kernel, Xt[rows]) - np.sum(V * V, axis=0) + g.getnoise()
        assert np.allclose(mu_l[ptr[j]:ptr[j + 1]], mo, rtol=RTOL, atol=1e-9)
        assert np.allclose(var_l[ptr[j]:ptr[j + 1]], vo, rtol=RTOL, atol=1e-10)
        del C, V, Knt, g
    # properties of the whole model
    m0 = model.leaf_mll.copy()
    assert np.all(np.isfinite(model.leaf_mll)) and np.all(model.leaf_info == 0)
    assert abs(z - dsm.mll(model)) <= 1e-9 * abs(z)                        # update! returns the tree mll
    noise = np.exp(2 * np.log(0.1))
    assert np.all(var_l > noise) and np.all(var_l < 1.0 + noise + 1e-9)    # prior variance bounds per leaf
    assert np.all(var > noise * 0.999)                                     # law of total variance keeps the noise floor
    cnt = np.diff(ptr)
    assert cnt.sum() == 9 * Xt.shape[0]                                    # V^depth leaves per test row
    # the mixture mean lies between the extreme leaf means of each row
    lo = np.full(Xt.shape[0], np.inf)
    hi = np.full(Xt.shape[0], -np.inf)
    np.minimum.at(lo, idx, mu_l)
    np.maximum.at(hi, idx, mu_l)
    assert np.all(mu >= lo - 1e-9) and np.all(mu <= hi + 1e-9)
    # refit is idempotent (bit-reproducible schedule, no atomics); the test set is resident now, so both fits
    # below take the joint path (a different split-K schedule than the first fit: last-bit differences only)
    dsm.fit(model)
    m1 = model.leaf_mll.copy()
    assert np.allclose(m1, m0, rtol=1e-12)                                # joint path against the first (plain) fit
    dsm.fit(model)
    assert np.array_equal(m1, model.leaf_mll)
    mu2, var2 = dsm.predict(model, Xt)
    assert np.allclose(mu2, mu, rtol=1e-10, atol=1e-12) and np.allclose(var2, var, rtol=1e-9, atol=1e-13)
    rmse = np.sqrt(np.mean((mu - (np.mean([np.sin(2 * np.pi * (d + 1) * Xt[:, d]) for d in range(8)], axis=0))) ** 2))
    assert rmse < 0.35                                                     # bounded error against the noiseless target


def test_config5_scaled_kernel_vector_training():
    """BASELINE config 5 scaled to oracle size: KernelFunction[IsoSE, IsoLinear], D=16, train!(ADAM) loop -- the
    per-kernel-id hyper-vector, sum-over-GPs weights (infer!) and the gradient back-propagation through them."""
    N, D = 4000, 16
    X, y, Xt = regression_data(N, D, n_test=100, seed=20205)
    kv = [dsm.IsoSE(np.log(1.0), 0.0), dsm.IsoLinear(np.log(2.0))]
    m = dsm.buildDSMGP(X, y, 3, 4, M=150, kernel=kv, logNoise=np.log(0.3), seed=5)
    h0 = dsm.getparams(m).copy()
    _, hist = dsm.train(m, dsm.ADAM(eta=0.01), iterations=3, randinit=False)
    hyp = h0.copy()
    opt = dsm.ADAM(eta=0.01)
    ref = []
    trained = dsm.getparams(m).copy()
    for it in range(3):
        dsm.setparams(m, hyp)
        gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
        ospn.fit_naive(m.root, gps)
        ref.append(ospn.mll(m.root, gps))
        hyp = hyp + opt.apply(hyp, ospn.grad_tree(m.root, gps, hyp.size))
    assert np.allclose(hist, ref, rtol=RTOL)
    assert np.allclose(trained, hyp, rtol=1e-9, atol=1e-12)
    dsm.setparams(m, trained)
    dsm.fit(m)
    zi = dsm.infer(m)
    gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
    ospn.fit_naive(m.root, gps)
    assert abs(zi - ospn.infer(m.root, gps)) <= RTOL * abs(zi)
    mu, var = dsm.predict(m, Xt)
    mo, vo = ospn.predict(m.root, gps, Xt)
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9) and np.allclose(var, vo, rtol=RTOL, atol=1e-10)


def test_concurrent_sub_contexts_give_the_single_context_result():
    """hipabi.MultiContext: the leaves of one GPU split over two contexts driven from two host threads
    (overlaps one context's panel phases with the other's update launches).  Per-leaf results are independent
    of the split, so everything matches the single-context model (last-bit differences from split-K schedules)."""
    X, y, Xt = regression_data(6000, 3, n_test=400, seed=555)
    kw = dict(M=80, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=5)
    m1 = dsm.buildDSMGP(X, y, 3, 4, **kw)
    m2 = dsm.buildDSMGP(X, y, 3, 4, n_sub=2, **kw)
    assert isinstance(m2.ctx, hipabi.MultiContext) and all(len(p) > 0 for p in m2.ctx.part)
    assert np.allclose(m1.leaf_mll, m2.leaf_mll, rtol=1e-12)
    z1, z2 = dsm.update(m1), dsm.update(m2)
    assert abs(z1 - z2) <= 1e-11 * abs(z1)
    for _ in range(2):                       # second round: test rows ride through fit in both models
        a, b = dsm.predict(m1, Xt), dsm.predict(m2, Xt)
        assert np.allclose(a[0], b[0], rtol=1e-10, atol=1e-12) and np.allclose(a[1], b[1], rtol=1e-9, atol=1e-13)
        dsm.fit(m1)
        dsm.fit(m2)
    dsm.updategradients(m1)
    dsm.updategradients(m2)
    assert np.allclose(dsm.grad_mll(m1), dsm.grad_mll(m2), rtol=1e-9, atol=1e-10)
    # more contexts than leaves: the spare ones stay idle
    g = dsm.GaussianProcess(X[:500], y[:500], kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1))
    mc = hipabi.MultiContext(0, 3)
    mc.set_train(X[:500], y[:500])
    mc.set_leaves(np.array([0, 500]), np.arange(500), [0], [float(np.mean(y[:500]))])
    mc.set_hyper(0, 0, [np.log(0.3), 0.0, np.log(0.1)])
    mll, info, _ = mc.fit()
    assert len(mc.act) == 1 and info[0] == 0
    dsm.update_cholesky(g)
    assert abs(mll[0] - dsm.mll(g)) <= 1e-10 * abs(mll[0])
    mc.close()


def test_streaming_factor_and_discard_equals_resident():
    """hipabi.StreamingContext: leaf groups under a byte budget, factors discarded after each group.  Same
    log-marginals, predictions and gradients as the resident model (the mode config 5 needs)."""
    X, y, Xt = regression_data(6000, 3, n_test=400, seed=556)
    kw = dict(M=80, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=5)
    m1 = dsm.buildDSMGP(X, y, 3, 4, **kw)
    n = np.array([lf.nobs for lf in m1.leaves])
    budget = int(0.3 * hipabi.estimate_bytes(n, np.full(n.size, 400 * 9 // n.size + 1), 3, True))
    m2 = dsm.buildDSMGP(X, y, 3, 4, stream_budget=budget, **kw)
    assert isinstance(m2.ctx, hipabi.StreamingContext) and len(m2.ctx.groups) >= 2
    assert np.allclose(m1.leaf_mll, m2.leaf_mll, rtol=1e-12)
    dsm.update(m1)
    dsm.update(m2)
    a, b = dsm.predict(m1, Xt), dsm.predict(m2, Xt)
    assert np.allclose(a[0], b[0], rtol=1e-10, atol=1e-12) and np.allclose(a[1], b[1], rtol=1e-9, atol=1e-13)
    p0 = m2.ctx.passes
    b2 = dsm.predict(m2, Xt)                                  # cached: no new pass over the groups
    assert m2.ctx.passes == p0 and np.array_equal(b[0], b2[0])
    dsm.updategradients(m1)
    dsm.updategradients(m2)
    assert np.allclose(dsm.grad_mll(m1), dsm.grad_mll(m2), rtol=1e-9, atol=1e-10)
    assert len(m2.ctx.groups) >= 3                            # L^-1 and the test rows count against the budget
    _, h1 = dsm.train(m1, dsm.ADAM(eta=0.01), iterations=2, randinit=False)
    _, h2 = dsm.train(m2, dsm.ADAM(eta=0.01), iterations=2, randinit=False)
    assert np.allclose(h1, h2, rtol=1e-10)
    # a copy-sharing model (config 1) streams too: leaves that alias a factor stay in one group
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "config1.npz"))
    mc = dsm.buildDSMGP(z["x"].reshape(-1, 1), z["y"], 3, 4, M=10, kernel=dsm.IsoSE(1.0, 1.0), meanFun=dsm.ConstMean(0.5),
                        seed=11, stream_budget=6 << 20)
    assert len(mc.ctx.groups) >= 2 and np.allclose(mc.leaf_mll, z["leaf_mll"], rtol=RTOL, atol=1e-9)


def test_reference_self_check_construction_through_the_hip_path(ctx, golden_dir):
    """The only executable checks the reference holds for this path -- src/AdvancedCholeskey.jl test_chol_continue
    (:121-135: potrf of the leading P x P block, chol_continue! from column P+1, compare with cholesky) and lrtest
    (:61-110: genCov matrix with ten rows removed, compare with cholesky of the reduced matrix) -- rebuilt with the
    portable generator (tests/golden/make_advchol.py) and pushed through the C ABI: the genCov matrix Sigma becomes
    the Gram matrix of an IsoLinear leaf (K_y = X X^T + 1 with X = chol(Sigma - I), l = 1, noise + eps = 1), the
    leading block is a source leaf and the whole matrix a PREFIX leaf (= chol_continue!), the reduced matrix a leaf
    over the kept rows.  Expected factors: LAPACK dpotrf, mpmath-checked (fixture advchol.npz)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_advchol", os.path.join(golden_dir, "make_advchol.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z = np.load(os.path.join(golden_dir, "advchol.npz"))
    logn = 0.5 * np.log(1.0 - 1e-8)                     # exp(2 logNoise) + 1e-8 == 1
    for name in ("cont_d100_p10", "cont_d192_p150"):
        D, P, seed = int(z[f"{name}/D"]), int(z[f"{name}/P"]), int(z[f"{name}/seed"])
        S = mod.gen_cov(D, seed)
        X = np.linalg.cholesky(S - np.eye(D))
        ctx.set_train(X, np.zeros(D))
        ctx.set_leaves([0, P, P + D], np.concatenate([np.arange(P), np.arange(D)]), [0, 0], [0.0, 0.0])
        ctx.set_hyper(0, 2, [0.0, 0.0, logn])
        ctx.set_sharing([0, 2], [-1, 0], [0, P])        # leaf 1 continues leaf 0's factor from column P+1
        mll, info, _ = ctx.fit()
        assert info[0] == 0 and info[1] == 0
        F, _ = ctx.download_factor(1, D)
        Lref = z[f"{name}/L"]
        assert np.max(np.abs(F - Lref)) <= 1e-12 * np.max(np.abs(Lref)), name
        assert np.sum(np.abs(F - Lref)) < 1e-9           # the quantity test_chol_continue returns (:134)
        F0, _ = ctx.download_factor(0, P)
        assert np.max(np.abs(F0 - Lref[:P, :P])) <= 1e-12 * np.max(np.abs(Lref))
        # y = 0: alpha = 0 and mll = -(logdet + n log 2pi)/2
        assert abs(mll[1] + (2 * np.sum(np.log(np.diag(Lref))) + D * np.log(2 * np.pi)) / 2) <= 1e-10 * abs(mll[1])
    D, seed = int(z["lr/D"]), int(z["lr/seed"])
    A = mod.gen_cov(D, seed)
    idx = np.setdiff1d(np.arange(D), z["lr/missing"])
    X = np.linalg.cholesky(A - np.eye(D))
    ctx.set_train(X, np.zeros(D))
    ctx.set_leaves([0, D, D + idx.size], np.concatenate([np.arange(D), idx]), [0, 0], [0.0, 0.0])
    ctx.set_hyper(0, 2, [0.0, 0.0, logn])
    ctx.set_sharing(None, None, None)                   # row deletion -> full factorisation
    mll, info, _ = ctx.fit()
    assert np.all(info == 0)
    for leaf, tag, n in ((0, "lr_A", D), (1, "lr_B", idx.size)):
        F, _ = ctx.download_factor(leaf, n)
        assert np.allclose(np.diag(F), z[f"{tag}/diag"], rtol=1e-12)
        assert abs(np.linalg.norm(F) - float(z[f"{tag}/fro"])) <= 1e-12 * float(z[f"{tag}/fro"])
        cols = z[f"{tag}/cols"]
        assert np.max(np.abs(F[:, cols] - z[f"{tag}/colvals"])) <= 1e-12 * np.max(np.abs(z[f"{tag}/colvals"]))
        assert abs(mll[leaf] + (float(z[f"{tag}/logdet"]) + n * np.log(2 * np.pi)) / 2) <= 1e-10 * abs(mll[leaf])


def test_environment_cannot_change_results(ctx):
    """The product library reads no tuning variables: DSMGP_TILE_V=101 used to route every
    factorisation through an ablation kernel with wrong results; now a context created under it is bit-identical."""
    X, y, _ = regression_data(1500, 3, n_test=8, seed=91)
    h = [np.log(0.3), 0.0, np.log(0.1)]
    ref, info, _ = _single(ctx, X, y, 0.0, 0, np.array(h[:2]), h[2])
    old = {k: os.environ.get(k) for k in ("DSMGP_TILE_V", "DSMGP_XCD", "DSMGP_TAIL_SPLIT")}
    os.environ.update(DSMGP_TILE_V="101", DSMGP_XCD="0", DSMGP_TAIL_SPLIT="7")
    try:
        c2 = hipabi.Context(0)
        got, info2, _ = _single(c2, X, y, 0.0, 0, np.array(h[:2]), h[2])
        c2.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert info[0] == 0 and info2[0] == 0 and got[0] == ref[0]


def test_config5_streaming_at_a_size_that_really_streams():
    """BASELINE config 5 at N = 250k, D = 16, M = 300, [IsoSE, IsoLinear]: 288 leaves, n = 3.8k..41.7k, 0.69 TB of
    factors -> the streaming context needs >= 2 leaf groups on a 288 GB GPU (the regime that defines config 5: pool reuse,
    npad^2 past int32, test rows riding through every group).  Checked against the oracle on the smallest leaves of both
    kernels, through K_y alpha = y on the LARGEST leaf of both kernels, and against a plain resident context on
    mid-size leaves."""
    import scipy.linalg as sla
    N, D = 250_000, 16
    X, y, Xt = regression_data(N, D, seed=20205)
    kern = [dsm.IsoSE(np.log(0.3), 0.0), dsm.IsoLinear(np.log(1.5))]
    m = dsm.buildDSMGP(X, y, 3, 4, M=300, D=2, kernel=kern, logNoise=np.log(0.1), seed=20205, fit_now=False,
                       stream_budget="auto")
    nobs = np.array([lf.nobs for lf in m.leaves])
    kind = np.array([lf.kernel.kind for lf in m.leaves])
    assert m.L == 288 and nobs.max() > 40_000
    big = [int(np.flatnonzero(kind == k)[np.argmax(nobs[kind == k])]) for k in (0, 2)]
    small = [int(np.flatnonzero(kind == k)[np.argmin(nobs[kind == k])]) for k in (0, 2)]
    m.ctx.keep_alpha = tuple(big)
    dsm.resident_test(m, Xt)
    dsm.fit(m)
    assert isinstance(m.ctx, hipabi.StreamingContext) and len(m.ctx.groups) >= 2
    assert np.all(m.leaf_info == 0) and np.all(np.isfinite(m.leaf_mll))
    z = dsm.infer(m)
    passes = m.ctx.passes
    mu, var = dsm.predict(m, Xt)
    assert m.ctx.passes == passes                          # the test rows rode through the fit pass
    assert np.isfinite(z) and np.all(np.isfinite(mu)) and np.all(var > 0)
    ptr, idx = m._route_cache["ptr"], m._route_cache["idx"]
    mu_l, var_l = m.ctx.predict_fetch()
    # smallest leaf of each kernel against the oracle
    for j in small:
        lf = m.leaves[j]
        g = ogp.GaussianProcess(X[lf.obs], y[lf.obs], lf.mean.m, ogp.make_kernel(lf.kernel.kind, lf.kernel.loghyp()),
                                lf.logNoise, exact_dist=True).update_cholesky()
        assert abs(m.leaf_mll[j] - g.mll()) <= RTOL * abs(g.mll())
        mo, vo = g.prediction(Xt[idx[ptr[j]:ptr[j + 1]]])
        assert np.allclose(mu_l[ptr[j]:ptr[j + 1]], mo, rtol=RTOL, atol=1e-9)
        assert np.allclose(var_l[ptr[j]:ptr[j + 1]], vo, rtol=RTOL, atol=1e-10)
    # largest leaf of each kernel: residual of K_y alpha = y - m, K_y assembled on the host in row blocks
    for j in big:
        lf = m.leaves[j]
        alpha = m.ctx.alpha(j)
        xs, yc = X[lf.obs], y[lf.obs] - lf.mean.m
        c = np.exp(2 * lf.logNoise) + 1e-8
        if lf.kernel.kind == 2:
            r = xs @ (xs.T @ alpha) / np.exp(2 * lf.kernel.logl) + c * alpha - yc
        else:
            l2, s2 = np.exp(2 * lf.kernel.logl), np.exp(2 * lf.kernel.logs)
            sq = np.sum(xs * xs, axis=1)
            r = np.empty(lf.nobs)
            for a in range(0, lf.nobs, 2048):
                P = np.maximum(sq[a:a + 2048, None] + sq[None, :] - 2.0 * (xs[a:a + 2048] @ xs.T), 0.0)
                r[a:a + 2048] = (s2 * np.exp(-0.5 * P / l2)) @ alpha
            r += c * alpha - yc
        assert np.max(np.abs(r)) <= 1e-7 * np.max(np.abs(yc)), (lf.nobs, lf.kernel.kind, np.max(np.abs(r)))
    # streamed == resident: six mid-size leaves refitted in a plain context (no pool, no groups)
    order = np.argsort(nobs)
    mid = [int(j) for j in order[140:146]]
    c2 = hipabi.Context(0)
    c2.set_train(X, y)
    lv = [m.leaves[j] for j in mid]
    c2.set_leaves(np.concatenate([[0], np.cumsum([lf.nobs for lf in lv])]), np.concatenate([lf.obs for lf in lv]),
                  [lf.kernelid for lf in lv], [lf.mean.m for lf in lv])
    for lf in m.kernel_table():
        c2.set_hyper(lf.kernelid, lf.kernel.kind, np.concatenate([lf.kernel.loghyp(), [lf.logNoise]]))
    mll2, info2, _ = c2.fit()
    c2.close()
    # a leaf's split-K schedule depends on which leaves share its launches: last-bit differences in the factor, amplified by
    # the conditioning of the rank-16 IsoLinear Gram (measured 5e-12 relative on its log-marginal)
    assert np.all(info2 == 0) and np.allclose(mll2, m.leaf_mll[mid], rtol=1e-10)


@pytest.mark.parametrize("family", ["dsmgp", "kernel_vector", "poe", "gpoe", "rbcm", "single_leaf"])
def test_device_aggregation_and_scores(family):
    """the sum/product aggregation of predict (src/common.jl:134-149,198-302) and the score functions
    (src/scorefunctions.jl:6-16) run on the moments resident in HBM (dsmgp_aggregate*, dsmgp_scores).  Against the
    oracle's literal recursions at 1e-8, against the host rules on the SAME moments at 1e-12 (they differ only in
    summation association), through the partial-sum path several contexts / ranks use, and the scores against the
    oracle's restatement."""
    from deepstructuredmixtures_amd import model as pmodel
    N, D = 2500, 3
    X, y, Xt = regression_data(N, D, n_test=333, seed=901)
    yt = np.mean([np.sin(2 * np.pi * (d + 1) * Xt[:, d]) for d in range(D)], axis=0)
    kern = dsm.IsoSE(np.log(0.3), 0.0)
    kw = dict(logNoise=np.log(0.1), seed=4)
    if family == "dsmgp":
        m = dsm.buildDSMGP(X, y, 3, 4, M=60, kernel=kern, **kw)
    elif family == "kernel_vector":
        m = dsm.buildDSMGP(X, y, 2, 4, M=60, kernel=[kern, dsm.IsoLinear(np.log(1.5))], **kw)
    elif family == "poe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), **kw)
    elif family == "gpoe":
        m = dsm.buildPoE(X, y, 8, M=100, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), generalized=True, **kw)
    elif family == "rbcm":
        m = dsm.buildBCM(X, y, 8, M=100, kernel=dsm.IsoLinear(np.log(0.7)), **kw)       # k(x*,x*) depends on the row
    else:
        m = dsm.buildBCM(X[:300], y[:300], 4, M=400, kernel=kern, **kw)
        assert m.L == 1
    Xn, yn = (X[:300], y[:300]) if family == "single_leaf" else (X, y)
    gps, _ = _oracle_model(m, Xn, yn)
    if m.family == "dsmgp":
        dsm.update(m)
        ospn.update(m.root, gps)
        mo, vo = ospn.predict(m.root, gps, Xt)
    elif m.root.kind == "gp" or m.family == "poe":
        mo, vo = ospn.predict_poe(m.root, gps, Xt)
    elif m.family == "gpoe":
        mo, vo = ospn.predict_gpoe(m.root, gps, Xt)
    else:
        mo, vo = ospn.predict_rbcm(m.root, gps, Xt)
    mu, var = dsm.predict(m, Xt)                              # device aggregation
    assert m._scores_on_device
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9), float(np.max(np.abs(mu - mo)))
    assert np.allclose(var, vo, rtol=RTOL, atol=1e-10), float(np.max(np.abs(var - vo) / vo))
    # host rules on the same moments
    rc = pmodel._routing(m, np.asfortranarray(Xt))           # the host's lists (the context routed the rows itself: same CSR)
    mu_l, var_l = m.ctx.predict_fetch()
    if m.family == "dsmgp":
        mh, vh = pmodel._aggregate_dsmgp_flat(m, Xt.shape[0], rc, mu_l, var_l)
        mr, vr = pmodel._aggregate_dsmgp(m, np.asfortranarray(Xt), rc["ptr"], mu_l, var_l)
        assert np.allclose(mu, mr, rtol=1e-12, atol=1e-13) and np.allclose(var, vr, rtol=1e-9, atol=1e-13)
    else:
        mh, vh = pmodel._aggregate_poe(m, np.asfortranarray(Xt), rc["ptr"], mu_l, var_l)
    assert np.allclose(mu, mh, rtol=1e-12, atol=1e-13) and np.allclose(var, vh, rtol=1e-11, atol=1e-14)
    # partial sums + finish (what several ranks / contexts do), device finish and host finish
    fam, coef, group, G, plain, prior = pmodel._aggregation_spec(m)
    part = m.ctx.aggregate_partial(fam, coef, group, G)
    assert part.shape == (hipabi.agg_width(fam, G), Xt.shape[0])
    m1, v1 = m.ctx.aggregate_finish(None, plain=plain, prior_kernel_id=prior.kernelid if prior else 0)
    assert np.array_equal(m1, mu) and np.array_equal(v1, var)
    half = 0.5 * part
    m2, v2 = m.ctx.aggregate_finish(half + half, plain=plain, prior_kernel_id=prior.kernelid if prior else 0)
    assert np.array_equal(m2, mu) and np.array_equal(v2, var)
    m3, v3 = pmodel._finish_partial(m, np.asfortranarray(Xt), fam, part, G, plain, prior)
    assert np.allclose(m3, mu, rtol=1e-13, atol=1e-15) and np.allclose(v3, var, rtol=1e-12, atol=1e-15)
    # scores of the resident prediction against the oracle's restatement of scorefunctions.jl
    sc = dsm.scores(m, yt)
    ref = dict(mse=oscores.mse(yt, mo), sse=oscores.sse(yt, mo), mae=oscores.mae(yt, mo), sae=oscores.sae(yt, mo),
               nlpd=oscores.nlpd(yt, mo, vo))
    for k, v in ref.items():
        assert abs(sc[k] - v) <= RTOL * max(1.0, abs(v)), (k, sc[k], v)
    host = dsm.scores(m, yt, mu, var)
    assert all(abs(host[k] - sc[k]) <= 1e-12 * max(1.0, abs(sc[k])) for k in sc)
    if family == "dsmgp":      # the same model over two concurrent contexts: partial sums of the sub-contexts, host finish
        m2c = dsm.buildDSMGP(X, y, 3, 4, M=60, kernel=kern, n_sub=2, **kw)
        dsm.update(m2c)
        mu2, var2 = dsm.predict(m2c, Xt)
        assert not m2c._scores_on_device
        assert np.allclose(mu2, mu, rtol=1e-11, atol=1e-12) and np.allclose(var2, var, rtol=1e-9, atol=1e-13)


def test_aggregate_error_paths(ctx):
    X, y, Xt = regression_data(600, 2, n_test=20, seed=17)
    ctx.set_train(X, y)
    ctx.set_leaves([0, 300, 600], np.arange(600), [0, 0], [0.0, 0.0])
    ctx.set_sharing(None, None, None)
    ctx.set_hyper(0, 0, [np.log(0.3), 0.0, np.log(0.1)])
    ctx.fit()
    with pytest.raises(hipabi.DsmgpError):
        ctx.aggregate(hipabi.AGG_POE, np.ones(2))                     # no prediction yet
    ctx.predict_leaves(Xt, [0, 20, 40], np.tile(np.arange(20), 2))
    with pytest.raises(hipabi.DsmgpError):
        ctx.scores(np.zeros(20))                                      # no aggregation yet
    with pytest.raises(hipabi.DsmgpError):
        ctx.aggregate(7, np.ones(2))
    with pytest.raises(hipabi.DsmgpError):
        ctx.aggregate(hipabi.AGG_RBCM, None, np.array([0, 5], dtype=np.int32), 2)   # group out of range
    mu, var = ctx.aggregate(hipabi.AGG_POE, np.ones(2))
    ml, vl = ctx.predict_fetch()
    t = 1 / vl.reshape(2, 20)
    assert np.allclose(var, 1 / t.sum(0), rtol=1e-14) and np.allclose(mu, (t * ml.reshape(2, 20)).sum(0) / t.sum(0), rtol=1e-13)


def test_throughput_and_latency_forms_of_the_diagonal_block_kernel_agree(ctx):
    """The diagonal-block kernel (75 KB packed LDS image, L^-1 formed block column by block column in registers after L,
    forward substitution riding along, pure-padding block steps skipped) in launches of every kind -- 600 blocks per launch
    (two workgroups per CU, fused steps: the tile arrives in the image straight from its update) against the same leaves
    fitted 100 at a time (fewer blocks than CUs; until round 3 a second, 147 KB "latency" form of the kernel ran there):
    same factors, inverses (through alpha and the prediction) and fused forward solves, to rounding; a sample against the
    oracle.  Leaves of 140..330 rows: last blocks of 12..128 data rows."""
    N, D, L = 40_000, 3, 600
    X, y, Xt = regression_data(N, D, n_test=40, seed=4711)
    rng = np.random.default_rng(3)
    sizes = rng.integers(140, 331, size=L)
    obs = [np.sort(rng.choice(N, size=int(n), replace=False)) for n in sizes]
    hyp = [np.log(0.3), 0.0, np.log(0.1)]

    def run(sel):
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([obs[j].size for j in sel])]), np.concatenate([obs[j] for j in sel]),
                       np.zeros(len(sel), dtype=np.int32), [float(np.mean(y[obs[j]])) for j in sel])
        ctx.set_sharing(None, None, None)
        ctx.set_hyper(0, 0, hyp)
        mll, info, _ = ctx.fit()
        assert np.all(info == 0)
        nt = Xt.shape[0]
        mu, var = ctx.predict_leaves(Xt, np.arange(len(sel) + 1) * nt, np.tile(np.arange(nt), len(sel)))
        alphas = [ctx.download_factor(i, obs[j].size)[1] for i, j in enumerate(sel[:5])]
        return mll, mu.reshape(len(sel), nt), var.reshape(len(sel), nt), alphas

    big = run(list(range(L)))                                   # 600 blocks per launch > 256 CUs
    for a in range(0, L, 100):                                  # 100 blocks per launch
        sel = list(range(a, a + 100))
        small = run(sel)
        assert np.allclose(big[0][a:a + 100], small[0], rtol=1e-12)
        assert np.allclose(big[1][a:a + 100], small[1], rtol=1e-11, atol=1e-12)
        assert np.allclose(big[2][a:a + 100], small[2], rtol=1e-10, atol=1e-13)
        if a == 0:
            for u, v in zip(big[3], small[3]):
                assert np.allclose(u, v, rtol=1e-10, atol=1e-12)
    for j in (0, 299, 599):
        g = ogp.GaussianProcess(X[obs[j]], y[obs[j]], float(np.mean(y[obs[j]])), ogp.IsoSE(hyp[0], hyp[1]), hyp[2], True).update_cholesky()
        assert abs(big[0][j] - g.mll()) <= RTOL * abs(g.mll())
        mo, vo = g.prediction(Xt)
        assert np.allclose(big[1][j], mo, rtol=RTOL, atol=1e-9) and np.allclose(big[2][j], vo, rtol=RTOL, atol=1e-10)


def test_bench_two_ranks_on_one_gpu_matches_one_rank(tmp_path):
    """bench.py's N > 1 path, rehearsed on this one GPU: two ranks under torch.distributed.run with the
    gloo backend (DSMGP_BENCH_BACKEND=gloo; the launcher starts before anything touches the GPU), each with its leaf
    shard in its own HIP contexts.  The JSON line must carry n_gpus = 2, a finite value and the root log-marginal of
    the one-rank run."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--config", "dsmgp_n20k_d8", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # --full: the one-rank line below also carries the probe, the drop-in series and the probe-relative roofline
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--full", "--dump-outputs", str(tmp_path / "one")]
                         + common, env=env, capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stderr[-2000:]
    j1 = json.loads(one.stdout.strip().splitlines()[-1])
    # --dump-outputs: what the last timed step returned (predictive moments, root and leaf log-marginals), float64
    d1 = {k: np.load(tmp_path / "one" / f"{k}.npy") for k in ("mu", "var", "root_mll", "leaf_mll")}
    # (the line's root_mll is the one of the untimed steps after the timed loop: the same value up to summation order)
    assert all(a.dtype == np.float64 for a in d1.values()) and abs(d1["root_mll"][0] - j1["root_mll"]) <= 1e-10 * abs(j1["root_mll"])
    assert d1["mu"].shape == d1["var"].shape == (2000,) and np.all(d1["var"] > 0) and d1["leaf_mll"].shape == (144,)
    # `python bench.py --gpus 2` with NO launcher (the shape of the driver's N = 1 command; VERDICT r4 #5a): the process starts its
    # own two ranks under torch.distributed.run before touching the GPU and relays rank 0's line (it used to die on an assert)
    env_nolaunch = {k: v for k, v in env.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    two = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dump-outputs", str(tmp_path / "two")] + common,
                         env=dict(env_nolaunch, DSMGP_BENCH_BACKEND="gloo"), capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-3000:]
    assert "without a launcher" in two.stderr
    d2 = {k: np.load(tmp_path / "two" / f"{k}.npy") for k in ("mu", "var", "root_mll", "leaf_mll")}
    assert np.allclose(d2["mu"], d1["mu"], rtol=RTOL, atol=1e-10) and np.allclose(d2["var"], d1["var"], rtol=RTOL, atol=1e-12)
    assert np.allclose(d2["leaf_mll"], d1["leaf_mll"], rtol=RTOL, atol=0)
    line = [ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1]
    j2 = json.loads(line)
    assert j1["n_gpus"] == 1 and j2["n_gpus"] == 2 and j2["scaling"] == "strong"
    assert np.isfinite(j2["value"]) and j2["value"] > 0 and j2["unit"] == "s" and j2["metric"] == j1["metric"]
    assert abs(j2["root_mll"] - j1["root_mll"]) <= 1e-10 * abs(j1["root_mll"])
    assert "roofline" in j1 and "standalone_predict_s" in j1 and j1["roofline"]["bound"] == "mfma"
    # the line explains itself: per-step spread, the f64-MFMA probe before warm-up and right after the timed loop, the shader
    # clock held inside the steps, the drop-in series (VERDICT r4 #1b, #7) ...
    assert j1["step_s"]["min"] <= j1["step_s"]["median"] <= j1["step_s"]["max"] and j1["drop_in_s"]["median"] > 0
    assert j1["f64_mfma_probe"]["before_warmup"]["tflops"] > 30 and j1["f64_mfma_probe"]["after_timed_loop"]["tflops"] > 30
    assert 1.0 < j1["roofline"]["clock_ghz_in_steps"] < 3.0 and 0 < j1["roofline"]["frac_of_probe"] < 1.2
    # ... and per rank what it held and how long it waited (#5b)
    assert j2["exchange_backend"] == "gloo" and [r["rank"] for r in j2["ranks"]] == [0, 1]
    assert abs(sum(r["cholesky_flop_share"] for r in j2["ranks"]) - 1.0) < 1e-12 and all(r["n_leaves"] > 0 for r in j2["ranks"])
    assert all(r["exchanges_per_step"] >= 2 and r["exchange_s_per_step"] > 0 for r in j2["ranks"])
    # the same launch as the driver's (no backend override): RCCL cannot come up with two ranks on this one GPU, and the run
    # must say so and complete over gloo instead of dying -- on every rank alike
    port = str(31000 + (os.getpid() * 7) % 2000)
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", port, os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         env=env, capture_output=True, text=True, timeout=900)
    assert two.returncode == 0, two.stderr[-3000:]
    j3 = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1])
    assert j3["n_gpus"] == 2 and j3["exchange_backend"] == "gloo" and "falling back to gloo" in two.stderr
    assert abs(j3["root_mll"] - j1["root_mll"]) <= 1e-10 * abs(j1["root_mll"])


def test_rccl_allgather_entry_point(ctx):
    """The C entry a Julia host binds for the multi-GPU exchange (dsmgp_comm_unique_id / dsmgp_comm_init /
    dsmgp_allgather over RCCL, librccl.so opened with dlopen on first use).  One GPU here, so a one-rank communicator:
    checks that the library loads, the communicator comes up on the context's device and stream, and the gathered
    block is the sent block; RCCL refuses two ranks on one GPU, the two-rank path is rehearsed over gloo
    (test_two_ranks_..., test_bench_two_ranks_...)."""
    ctx.world = 1
    with pytest.raises(hipabi.DsmgpError):
        ctx.allgather(np.zeros(4))                                 # before comm_init
    uid = hipabi.Context.comm_unique_id()
    assert len(uid) == 128 and any(b != 0 for b in uid)
    ctx.comm_init(0, 1, uid)
    try:
        with pytest.raises(hipabi.DsmgpError):
            ctx.comm_init(0, 1, uid)                               # already initialised
        v = np.sin(np.arange(5000.0))
        out = ctx.allgather(v)
        assert out.shape == (1, 5000) and np.array_equal(out[0], v)
        out = ctx.allgather(v[:7])                                 # smaller message: staging buffer reused
        assert np.array_equal(out[0], v[:7])
    finally:
        ctx.comm_destroy()


def test_copy_leaves_share_their_gradient_contraction():
    """SURVEY 8(f).4, the shared-gradient idea of src/fit.jl:313-395: a leaf whose observation set equals its main
    leaf's takes that leaf's gradients (`copygradients`, :352-356).  Here a COPY leaf (same factor, same kernel id, same
    ConstMean) skips its contraction tiles and reads its source's sum.  BASELINE config 1 has many such leaves: the
    gradients with sharing equal those of the naive schedule (every leaf on its own) and the oracle's."""
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "config1.npz"))
    X, y = z["x"].reshape(-1, 1), z["y"]
    kw = dict(M=10, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.2), seed=11)
    m = dsm.buildDSMGP(X, y, 3, 4, **kw)
    assert np.count_nonzero(m.share_op == ptree.SHARE_COPY) > 3
    g_shared = dsm.updategradients(m).copy()
    grad_shared = dsm.grad_mll(m)
    dsm.fit_naive(m)
    g_naive = dsm.updategradients(m).copy()
    assert np.allclose(g_shared, g_naive, rtol=1e-9, atol=1e-11)
    assert np.allclose(grad_shared, dsm.grad_mll(m), rtol=1e-9, atol=1e-11)
    gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
    ospn.fit_naive(m.root, gps)
    go = np.array([g.grad() for g in gps])
    assert np.allclose(g_shared, go, rtol=1e-7, atol=1e-8)
    # a COPY leaf with a mean of its own must NOT share (its alpha differs): two leaves over the same rows, means 0 and 1
    c = hipabi.Context(0)
    Xs, ys, _ = regression_data(300, 2, n_test=4, seed=5)
    c.set_train(Xs, ys)
    c.set_leaves([0, 300, 600], np.tile(np.arange(300), 2), [0, 0], [0.0, 1.0])
    c.set_hyper(0, 0, [np.log(0.4), 0.0, np.log(0.2)])
    c.set_sharing([0, 1], [-1, 0], [0, 0])
    c.fit()
    g2 = c.gradients(3)
    c.set_sharing(None, None, None)
    c.fit()
    g2n = c.gradients(3)
    c.close()
    assert np.allclose(g2, g2n, rtol=1e-9, atol=1e-11) and abs(g2[0, 0] - g2[1, 0]) > 1e-6


def test_ardse_true_lengthscale_gradient_option(ctx):
    """the reference's ArdSE length-scale gradients are identically zero (a parse accident) and
    that is the default here too.  dsmgp_set_option(DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT, 1) switches to the true
    derivative of the log-marginal w.r.t. log l_d of the additive kernel: checked against central finite differences of
    the device's own log-marginal; ds and dnoise do not change with the option."""
    n, D = 420, 3
    X = uniform(95, 0, n * D).reshape((n, D), order="F")
    y = np.sin(4 * X[:, 0]) + np.cos(3 * X[:, 1]) + 0.1 * normal(96, 0, n)
    h = np.array(list(np.log([0.4, 0.6, 0.9])) + [0.1])
    ln = np.log(0.25)
    mean = float(np.mean(y))
    _single(ctx, X, y, mean, 1, h, ln)
    g0 = ctx.gradients(D + 2)[0]
    assert np.all(g0[:D] == 0.0)
    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
    try:
        g1 = ctx.gradients(D + 2)[0]
        assert g1[D] == g0[D] and g1[D + 1] == g0[D + 1]
        eps = 1e-5
        for d in range(D):
            hp, hm = h.copy(), h.copy()
            hp[d] += eps
            hm[d] -= eps
            fp = _single(ctx, X, y, mean, 1, hp, ln)[0][0]
            fm = _single(ctx, X, y, mean, 1, hm, ln)[0][0]
            fd = (fp - fm) / (2 * eps)
            assert abs(g1[d] - fd) <= 2e-6 * max(1.0, abs(fd)), (d, g1[d], fd)
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    _single(ctx, X, y, mean, 1, h, ln)
    assert np.all(ctx.gradients(D + 2)[0][:D] == 0.0)


def test_bench_train_mode_line(tmp_path):
    """`bench.py --mode train` on the small config: one JSON line with the device split of a train! iteration and the
    rooflines of the two gradient passes; the log-marginal rises under the ascent steps.  --dump-outputs writes the last
    timed iteration's log-marginal, gradient and updated hyper-parameters."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--mode", "train", "--config", "dsmgp_n20k_d8", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["metric"].startswith("train! iteration") and j["unit"] == "s" and j["value"] > 0 and j["higher_is_better"] is False
    dev = j["device_seconds_per_iteration"]
    assert dev["grad_inverse"] > 0 and dev["grad_contraction"] > 0 and dev["total_fit"] > 0
    assert 0 < j["roofline"]["frac"] < 1 and 0 < j["roofline_inverse"]["frac"] < 1
    assert len(j["mll_history"]) == 3 and j["mll_history"][-1] > j["mll_history"][0]
    d = {k: np.load(tmp_path / f"{k}.npy") for k in ("mll", "gradient", "hyperparameters")}
    assert d["mll"].tolist() == [j["mll_history"][-1]] and d["gradient"].shape == d["hyperparameters"].shape
    assert np.all(np.isfinite(d["gradient"])) and np.any(d["gradient"] != 0)


@pytest.mark.gpu
def test_gram_fused_into_the_update_tasks_equals_the_gram_launch():
    """DSMGP_OPT_FUSED_GRAM (default on): the update tasks evaluate the kernel function for their tile with the operations
    of the Gram launch in the same order, so a factor whose tiles were not split along K comes out bit for bit the same
    as with every tile written by the Gram launch first; split tiles sum `product - Gram` instead of `Gram - product`
    (rounding only).  All three kernel kinds, COPY / PREFIX leaves, test rows riding along, padding-row tiles."""
    X, y, Xt = regression_data(6000, 4, n_test=500, seed=4321)
    cases = [lambda **kw: dsm.buildDSMGP(X, y, 3, 4, M=120, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=8, **kw),
             lambda **kw: dsm.buildPoE(X, y, 4, M=700, kernel=dsm.ArdSE(np.log([0.3, 0.4, 0.5, 0.6]), 0.0), logNoise=np.log(0.2),
                                       meanFun=dsm.ConstMean(0.1), seed=8, **kw),
             lambda **kw: dsm.buildDSMGP(X, y, 2, 3, M=400, D=1, kernel=[dsm.IsoSE(np.log(0.4), 0.0), dsm.IsoLinear(np.log(2.0))],
                                         logNoise=np.log(0.3), seed=5, **kw),
             lambda **kw: dsm.buildDSMGP(X[:3000], y[:3000], 2, 5, M=8, D=4, kernel=dsm.IsoSE(np.log(0.3), 0.0),
                                         logNoise=np.log(0.1), seed=9, **kw)]
    for make in cases:
        res = []
        for fused in (1, 0):
            m = make(fit_now=False)
            m.ctx.set_option(hipabi.OPT_FUSED_GRAM, fused)
            m.ctx.set_profile(True)
            dsm.resident_test(m, Xt)
            dsm.fit(m)
            t = m.ctx.timings()
            mu, var = dsm.predict(m, Xt)
            big = int(np.argmax([lf.nobs for lf in m.leaves]))
            F, alpha = m.ctx.download_factor(big, m.leaves[big].nobs)
            res.append((m.leaf_mll.copy(), mu, var, np.tril(F), alpha, t["gram"], m.share_op.copy()))
            assert np.all(m.leaf_info == 0)
        (ml1, mu1, v1, F1, a1, g1, op1), (ml0, mu0, v0, F0, a0, g0, op0) = res
        assert np.array_equal(op1, op0)
        assert np.allclose(ml1, ml0, rtol=1e-12, atol=1e-9)
        assert np.allclose(mu1, mu0, rtol=1e-10, atol=1e-11) and np.allclose(v1, v0, rtol=1e-9, atol=1e-12)
        assert np.allclose(F1, F0, rtol=1e-10, atol=1e-12) and np.allclose(a1, a0, rtol=1e-8, atol=1e-10)
        if max(lf.nobs for lf in m.leaves) > 1024:
            assert g1 < 0.8 * g0            # the Gram launch shrank to block column 0 (leaves of 9+ blocks: visible in its time)
    # a single GP of 8 blocks, one leaf per launch: every update launch has fewer tiles than CUs -> all split; and one
    # of 3 blocks next to it whose launches are not split on their own
    Xs, ys, _ = regression_data(1000, 3, n_test=10, seed=99)
    out = []
    for fused in (1, 0):
        c = hipabi.Context(0)
        c.set_option(hipabi.OPT_FUSED_GRAM, fused)
        c.set_train(Xs, ys)
        c.set_leaves(np.array([0, 1000]), np.arange(1000), [0], [float(ys.mean())])
        c.set_hyper(0, 0, [np.log(0.5), 0.0, np.log(0.2)])
        mll, info, _ = c.fit()
        F, alpha = c.download_factor(0, 1000)
        out.append((mll[0], np.tril(F), alpha))
        assert info[0] == 0
    assert abs(out[0][0] - out[1][0]) <= 1e-12 * abs(out[1][0])
    assert np.allclose(out[0][1], out[1][1], rtol=1e-11, atol=1e-13)
    Ky = out[1][1] @ out[1][1].T
    assert np.linalg.norm(out[0][1] @ out[0][1].T - Ky) <= 1e-14 * np.linalg.norm(Ky)


@pytest.mark.gpu
@pytest.mark.parametrize("D,kind", [(1, 0), (17, 0), (32, 0), (33, 0), (40, 1), (32, 1), (31, 2), (48, 2)])
def test_input_dimension_around_the_fused_gram_limit(ctx, D, kind):
    """The update tasks stage the coordinates of 128 rows and 128 columns through the ring's LDS up to D = 32
    (GRAM_FUSE_MAX_D); above that fit! falls back to the Gram launch for every tile.  Both sides of the limit, every
    kernel kind, a ragged leaf of 6 blocks with test rows riding along, against the oracle."""
    n, nt = 700, 150
    X = uniform(400 + D, 0, n * D).reshape((n, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.1 * normal(401 + D, 0, n)
    Xt = uniform(402 + D, 0, nt * D).reshape((nt, D), order="F")
    s = np.sqrt(D)                      # keep the kernel values away from 0 and 1 as D grows
    h = {0: [np.log(0.4 * s), 0.0], 1: list(np.log(np.linspace(0.3, 0.8, D))) + [0.1], 2: [np.log(0.9 * s), 0.0]}[kind]
    logNoise, mean = np.log(0.1), float(np.mean(y))
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [mean])
    ctx.set_hyper(0, kind, np.concatenate([h, [logNoise]]))
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    mll, info, _ = ctx.fit()
    g = ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, h), logNoise, exact_dist=True).update_cholesky()
    assert info[0] == 0 and g.info == 0
    assert abs(mll[0] - g.mll()) <= RTOL * max(1.0, abs(g.mll()))
    F, alpha = ctx.download_factor(0, n)
    assert np.max(np.abs(F - g.L())) <= 1e-9 * np.max(np.abs(g.L()))
    ctx.predict_run()
    mu, var = ctx.predict_fetch()
    mo, vo = g.prediction(Xt)
    assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9) and np.allclose(var, vo, rtol=RTOL, atol=1e-10)


@pytest.mark.gpu
def test_single_gp_prediction_registers_its_rows_once():
    """`prediction(gp, x)` (src/gaussianprocess.jl:110-137) on the host mirror keeps x registered (by content): the next
    `update_cholesky!` carries those rows through its launches and `prediction` on the same rows only finishes the
    moments; other rows are registered afresh.  Same numbers on every path, against the oracle."""
    X, y, Xt = regression_data(1500, 3, n_test=200, seed=31)
    h, ln = [np.log(0.4), 0.1], np.log(0.15)
    gp = dsm.GaussianProcess(X, y, kernel=dsm.IsoSE(*h), logNoise=ln)
    gp.model.ctx.set_profile(True)
    dsm.update_cholesky(gp)
    mu0, v0 = dsm.prediction(gp, Xt)                    # standalone sweep
    assert gp.model.ctx.timings()["predict_trsm"] > 0
    dsm.update_cholesky(gp)                             # Xt rides along
    mu1, v1 = dsm.prediction(gp, Xt)
    t = gp.model.ctx.timings()
    assert t["predict_update"] == 0.0 and t["predict_trsm"] == 0.0
    assert np.allclose(mu1, mu0, rtol=1e-11, atol=1e-12) and np.allclose(v1, v0, rtol=1e-10, atol=1e-13)
    go = ogp.GaussianProcess(X, y, float(np.mean(y)), ogp.IsoSE(*h), ln, True).update_cholesky()
    mo, vo = go.prediction(Xt)
    assert np.allclose(mu1, mo, rtol=RTOL, atol=1e-9) and np.allclose(v1, vo, rtol=RTOL, atol=1e-10)
    mu2, v2 = dsm.prediction(gp, Xt[:50])               # another test set: registered afresh
    mo2, vo2 = go.prediction(Xt[:50])
    assert np.allclose(mu2, mo2, rtol=RTOL, atol=1e-9) and np.allclose(v2, vo2, rtol=RTOL, atol=1e-10)
    mu3, v3 = dsm.predict(gp, Xt[:50])                  # predict(gp, x) clamps the variance like the tree models
    assert np.array_equal(mu3, mu2) and np.all(v3 > 0)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_fused_steps_agree_with_the_classic_steps(ctx, kind):
    """Small-leaf regime: a table of 700 leaves of 130..700 rows -- last row tiles of every class (<= 32,
    <= 64, <= 96, whole), 10..150 routed test rows per leaf (short and whole test tiles, two tiles for some), a COPY and
    a PREFIX leaf -- has more diagonal blocks per step than the chip has CUs, so its block steps run fused
    (diag_fused_reg_kernel + tile_fused8_kernel: each tile written once, short tiles in the 16-rows-per-wave form); with
    DSMGP_OPT_FUSED_STEPS = 0 the same table runs as update (short tiles in the column-split form) / packed diagonal
    block / panel solve launches.  Same arithmetic up to the order of one addition per entry: log-marginals 1e-12, the
    factor of sampled leaves 1e-11, moments 1e-9 (conditioning-limited); three leaves against the oracle at the
    north-star tolerance.  All three kernel kinds (the Gram values are evaluated inside the tasks)."""
    N, D, L = 60_000, 3, 700
    X, y, Xt = regression_data(N, D, n_test=160, seed=5150 + kind)
    rng = np.random.default_rng(11 + kind)
    sizes = rng.integers(130, 701, size=L)
    sizes[:8] = [130, 160, 192, 224, 256, 300, 352, 384]                  # every row class at least once
    obs = [np.sort(rng.choice(N, size=int(n), replace=False)) for n in sizes]
    obs[10] = obs[3].copy()                                               # COPY of leaf 3
    # a PREFIX claim needs the source's list as the leading part of an ascending list: rows above the source's last row
    tail = np.arange(obs[5][-1] + 1, min(N, obs[5][-1] + 1 + 230))
    obs[11] = np.concatenate([obs[5], tail])
    op = np.zeros(L, dtype=np.int32)
    src = np.full(L, -1, dtype=np.int32)
    plen = np.zeros(L, dtype=np.int64)
    op[10], src[10] = 1, 3
    if tail.size:
        op[11], src[11], plen[11] = 2, 5, obs[5].size
    ntest = rng.integers(10, 151, size=L)
    rptr = np.concatenate([[0], np.cumsum(ntest)])
    ridx = np.concatenate([np.sort(rng.choice(Xt.shape[0], size=int(k), replace=False)) for k in ntest])
    hyp = {0: [np.log(0.3), 0.0, np.log(0.1)], 1: [np.log(0.3), np.log(0.4), np.log(0.5), 0.0, np.log(0.1)],
           2: [np.log(1.5), 0.0, np.log(0.3)]}[kind]
    means = [float(np.mean(y[o])) for o in obs]
    means[10] = means[3]

    def run(fused):
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1 if fused else 0)
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, dtype=np.int32), means)
        ctx.set_sharing(op, src, plen)
        ctx.set_hyper(0, kind, hyp)
        ctx.set_test(Xt, rptr, ridx)                 # resident: the test rows ride through the factorisation launches
        ctx.set_profile(2)
        mll, info, _ = ctx.fit()
        t = ctx.timings()
        assert np.all(info == 0)
        ctx.predict_run()
        mu, var = ctx.predict_fetch()
        fa = [ctx.download_factor(j, obs[j].size) for j in (0, 5, 11, 300, 699, L - 1)]
        return mll, mu, var, fa, t

    try:
        a = run(True)
        b = run(False)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_profile(0)
    assert a[4]["gram"] < 0.5 * b[4]["gram"]           # no Gram launch: the tasks of block column 0 start from the kernel function
    assert np.allclose(a[0], b[0], rtol=1e-12, atol=0), float(np.max(np.abs(a[0] - b[0]) / np.abs(b[0])))
    # the moments carry the conditioning of K_y (1e5..1e6 here, more for the additive ArdSE kernel): two summation orders
    # of the same arithmetic agree to ~ cond x 1e-16, an order of magnitude inside the north-star tolerance
    emu = float(np.max(np.abs(a[1] - b[1])) / max(1.0, float(np.max(np.abs(b[1])))))
    evar = float(np.max(np.abs(a[2] - b[2]) / np.abs(b[2])))
    assert emu <= 1e-9 and evar <= 1e-9, (emu, evar)
    for (Fa, aa), (Fb, ab) in zip(a[3], b[3]):
        assert np.max(np.abs(Fa - Fb)) <= 1e-11 * np.max(np.abs(Fb)), float(np.max(np.abs(Fa - Fb)) / np.max(np.abs(Fb)))
        assert np.max(np.abs(aa - ab)) <= 1e-8 * np.max(np.abs(ab)), float(np.max(np.abs(aa - ab)) / np.max(np.abs(ab)))
    mk = {0: lambda: ogp.IsoSE(hyp[0], hyp[1]), 1: lambda: ogp.ArdSE(np.array(hyp[:3]), hyp[3]), 2: lambda: ogp.IsoLinear(hyp[0])}[kind]
    for j in (0, 11, 699):
        g = ogp.GaussianProcess(X[obs[j]], y[obs[j]], means[j], mk(), hyp[-1], True).update_cholesky()
        assert abs(a[0][j] - g.mll()) <= RTOL * abs(g.mll())
        mo, vo = g.prediction(Xt[ridx[rptr[j]:rptr[j + 1]]])
        assert np.allclose(a[1][rptr[j]:rptr[j + 1]], mo, rtol=RTOL, atol=1e-9)
        assert np.allclose(a[2][rptr[j]:rptr[j + 1]], vo, rtol=RTOL, atol=1e-10)


def test_fused_tile_tasks_pack_ragged_row_blocks(ctx):
    """The eight-wave fused tile task (round 4) packs ANY eight 16-row blocks below a diagonal block into one task: the last
    rows of a leaf's factor and its routed test rows share tasks, blocks hold 1..16 valid rows, the last task of a leaf is
    partly empty, the padding rows below the data are zeroed once per plan.  A table built from the edge cases -- leaf sizes
    one below / at / one above the multiples of 16 and of 128 (17 .. 640 rows: one to five block steps, all of them fused by
    the shallow rule), 0, 1, 15, 16, 17, 127, 128, 129 and 200 routed test rows, a leaf of ONE block (test blocks only), a
    COPY leaf whose test rows ride on its source's factor -- against the classic steps (update / diagonal block / panel solve
    launches) entry by entry, and every leaf against the oracle at the north-star tolerance."""
    N, D = 40_000, 3
    X, y, Xt = regression_data(N, D, n_test=256, seed=8642)
    rng = np.random.default_rng(97)
    edge_n = [17, 100, 127, 128, 129, 143, 144, 145, 159, 160, 161, 255, 256, 257, 271, 272, 273, 300, 383, 384, 385, 400, 511, 512, 513,
              527, 528, 529, 600, 639, 640]
    edge_t = [0, 1, 15, 16, 17, 100, 127, 128, 129, 200]
    sizes = [edge_n[i % len(edge_n)] for i in range(62)]
    ntest = [edge_t[(3 * i + i // len(edge_t)) % len(edge_t)] for i in range(62)]
    obs = [np.sort(rng.choice(N, size=int(n), replace=False)) for n in sizes]
    L = len(obs)
    obs[40] = obs[7].copy()                                               # COPY of leaf 7 (145 rows), with test rows of its own
    ntest[40], ntest[7] = 33, 0
    op = np.zeros(L, dtype=np.int32)
    src = np.full(L, -1, dtype=np.int32)
    plen = np.zeros(L, dtype=np.int64)
    op[40], src[40] = 1, 7
    rptr = np.concatenate([[0], np.cumsum(ntest)])
    ridx = np.concatenate([np.sort(rng.choice(Xt.shape[0], size=int(k), replace=False)) for k in ntest if k > 0])
    hyp = [np.log(0.3), 0.0, np.log(0.1)]
    means = [float(np.mean(y[o])) for o in obs]
    means[40] = means[7]

    def run(fused):
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1 if fused else 0)
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, dtype=np.int32), means)
        ctx.set_sharing(op, src, plen)
        ctx.set_hyper(0, 0, hyp)
        ctx.set_test(Xt, rptr, ridx)
        mll, info, _ = ctx.fit()
        assert np.all(info == 0)
        ctx.predict_run()
        mu, var = ctx.predict_fetch()
        fa = [ctx.download_factor(j, obs[j].size) for j in range(L)]
        return mll, mu, var, fa, ctx.work_fused()

    try:
        a = run(True)
        b = run(False)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
    assert a[4][1] > 0 and b[4][1] == 0                   # the first run did launch fused tile tasks, the second none
    assert np.allclose(a[0], b[0], rtol=1e-12, atol=0), float(np.max(np.abs(a[0] - b[0]) / np.abs(b[0])))
    assert float(np.max(np.abs(a[1] - b[1])) / max(1.0, float(np.max(np.abs(b[1]))))) <= 1e-9
    assert float(np.max(np.abs(a[2] - b[2]) / np.abs(b[2]))) <= 1e-9
    for (Fa, aa), (Fb, ab) in zip(a[3], b[3]):
        assert np.max(np.abs(Fa - Fb)) <= 1e-11 * np.max(np.abs(Fb))
        assert np.max(np.abs(aa - ab)) <= 1e-8 * np.max(np.abs(ab))
    for j in range(L):
        g = ogp.GaussianProcess(X[obs[j]], y[obs[j]], means[j], ogp.IsoSE(hyp[0], hyp[1]), hyp[-1], True).update_cholesky()
        assert abs(a[0][j] - g.mll()) <= RTOL * abs(g.mll()), j
        if ntest[j]:
            mo, vo = g.prediction(Xt[ridx[rptr[j]:rptr[j + 1]]])
            assert np.allclose(a[1][rptr[j]:rptr[j + 1]], mo, rtol=RTOL, atol=1e-9), j
            assert np.allclose(a[2][rptr[j]:rptr[j + 1]], vo, rtol=RTOL, atol=1e-10), j


def test_set_sharing_after_set_test_drops_the_test_set(ctx):
    """dsmgp_set_sharing rebuilds the leaf plan, so a test set registered before it (whose task lists point
    into the old plan's arenas) must go with it -- the C ABI sequence set_leaves -> set_test -> set_sharing -> fit used to
    replay the joint launches against freed memory.  Now the test set is dropped (predict says so), and registered again
    it gives the result of the unshared table."""
    N, D = 900, 2
    X, y, Xt = regression_data(N, D, n_test=50, seed=808)
    o = np.arange(0, 600)
    obs_ptr, obs_idx = [0, 600, 1200, 1500], np.concatenate([o, o, np.arange(600, 900)])
    means = [float(np.mean(y[o]))] * 2 + [float(np.mean(y[600:]))]
    rptr, ridx = np.arange(4) * 50, np.tile(np.arange(50), 3)

    def table():
        ctx.set_train(X, y)
        ctx.set_leaves(obs_ptr, obs_idx, [0, 0, 0], means)
        ctx.set_hyper(0, 0, [np.log(0.4), 0.0, np.log(0.2)])

    table()
    ctx.set_sharing(None, None, None)
    ctx.fit()
    ref = ctx.predict_leaves(Xt, rptr, ridx)
    table()
    ctx.set_test(Xt, rptr, ridx)
    ctx.set_sharing([0, 1, 0], [-1, 0, -1], [0, 0, 0])          # leaf 1 = COPY of leaf 0: new plan, new addresses
    mll, info, _ = ctx.fit()
    # (the COPY leaf's z comes from the forward sweep against Dinv_k, its source's from the substitution that rides in the
    # factorisation: the same value to rounding, not to the bit)
    assert np.all(info == 0) and abs(mll[0] - mll[1]) <= 1e-13 * abs(mll[0])
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.predict_run()
    assert "set_test" in str(e.value)
    ctx.set_test(Xt, rptr, ridx)
    ctx.fit()                                                   # joint: the rows ride through the new plan's launches
    ctx.predict_run()
    mu, var = ctx.predict_fetch()
    assert np.allclose(mu, ref[0], rtol=1e-11, atol=1e-12) and np.allclose(var, ref[1], rtol=1e-10, atol=1e-13)


def _edge_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "gp_edge.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    return cases


def test_mpmath_golden_across_a_tile_edge(ctx, golden_dir):
    """n = 160 crosses the 128-tile edge of the blocked factorisation (one whole block, a 32-row last tile, a panel solve
    and an update between them); test rows AT training inputs on both sides of the edge, 1e-7 away from them and elsewhere,
    noise standard deviation 0.03: sigma^2 = k** + noise - |V|^2 cancels three to four digits there.  50-digit mpmath
    values for all three kernel kinds (tests/golden/gp_edge.npz); the north-star tolerance with the fixture's small
    absolute term."""
    for name, c in _edge_cases(golden_dir).items():
        n = c["X"].shape[0]
        mll, info, _ = _single(ctx, c["X"], c["y"], float(c["mean"]), int(c["kind"]), c["loghyp"], float(c["logNoise"]))
        assert info[0] == 0
        assert abs(mll[0] - float(c["mll"])) <= RTOL * abs(float(c["mll"])), name
        _, alpha = ctx.download_factor(0, n)
        assert np.max(np.abs(alpha - c["alpha"])) <= 1e-7 * np.max(np.abs(c["alpha"])), name
        nt = c["Xt"].shape[0]
        mu, var = ctx.predict_leaves(c["Xt"], [0, nt], np.arange(nt))
        assert np.allclose(mu, c["mu"], rtol=RTOL, atol=1e-11), (name, float(np.max(np.abs(mu - c["mu"]))))
        assert np.allclose(var, c["var"], rtol=RTOL, atol=1e-11), (name, float(np.max(np.abs(var - c["var"]) / c["var"])))
        ctx.fit()                                                    # resident rows: the joint path gives the same numbers
        ctx.predict_run()
        mu2, var2 = ctx.predict_fetch()
        assert np.allclose(mu2, c["mu"], rtol=RTOL, atol=1e-11) and np.allclose(var2, c["var"], rtol=RTOL, atol=1e-11), name


def test_c_host_calls_the_abi(golden_dir, tmp_path):
    """tests/c_abi_smoke.c -- plain C99 against include/dsmgp_hip.h, no Python in the process -- runs create / set_train /
    set_leaves / set_hyper / fit / predict_leaves / download_factor / destroy on the mpmath-pinned n = 160 cases and
    compares with their numbers itself (exit code 0).  Built by __graft_entry__.build() (or here, when that could not); a
    child process, so its HIP context is its own."""
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "c_abi_smoke")
    if not os.path.exists(exe):       # build() tries, and does not fail the product build when it cannot: the failure belongs here
        import __graft_entry__
        __graft_entry__.build_c_host()
    for name, c in _edge_cases(golden_dir).items():
        n, D = c["X"].shape
        nt = c["Xt"].shape[0]
        hyp = np.concatenate([c["loghyp"], [float(c["logNoise"])]])
        path = os.path.join(tmp_path, name + ".bin")
        with open(path, "wb") as f:
            f.write(struct.pack("5q", n, D, nt, int(c["kind"]), hyp.size))
            for a in (np.asfortranarray(c["X"]).ravel(order="F"), c["y"], np.asfortranarray(c["Xt"]).ravel(order="F"), hyp,
                      np.array([float(c["mean"]), float(c["mll"])]), c["mu"], c["var"], c["alpha"]):
                f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stdout, r.stderr)
        assert "c_abi_smoke ok" in r.stdout and "gfx950" in r.stdout


def test_shard_exchange_through_the_library_communicator():
    """with the `nccl` process group the two exchanges of the path run inside the library -- per-leaf
    (mll, info) and the aggregation's partial sums are all-gathered device to device over RCCL on the context's stream
    (dsmgp_fit_exchange / dsmgp_aggregate_exchange) and only the results come to the host.  One GPU here, so a one-rank
    communicator (RCCL refuses two ranks on one device; the two-rank layout is rehearsed over gloo in the CPU suite):
    `Shard.device_comm(ctx, force=True)` drives fit!, update! and predict of a DSMGP and of an rBCM through that path;
    results must equal the plain single-context path bit for bit (a sum over one rank is the value itself)."""
    X, y, Xt = regression_data(4000, 3, n_test=300, seed=321)
    for build in (lambda: dsm.buildDSMGP(X, y, 3, 4, M=60, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=5, fit_now=False),
                  lambda: dsm.buildBCM(X, y, 4, M=300, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=5, fit_now=False)):
        ref = build()
        dsm.fit(ref)
        zr = dsm.update(ref) if ref.family == "dsmgp" else 0.0
        mr, vr = dsm.predict(ref, Xt)
        m = build()
        assert m.shard.device_comm(m.ctx, force=True) == "rccl-device" and m.shard.comm_ctx is m.ctx
        dsm.fit(m)
        z = dsm.update(m) if m.family == "dsmgp" else 0.0
        mu, var = dsm.predict(m, Xt)
        assert np.array_equal(m.leaf_mll, ref.leaf_mll) and np.array_equal(m.leaf_info, ref.leaf_info) and z == zr
        assert np.array_equal(mu, mr) and np.array_equal(var, vr)
        assert dsm.scores(m, np.zeros(Xt.shape[0])) == dsm.scores(ref, np.zeros(Xt.shape[0]))      # finish ran on the device
        # a second exchange of the same partial sums would add the total to itself `world` times: refused
        with pytest.raises(hipabi.DsmgpError):
            m.ctx.aggregate_exchange(3)
        # the rank-without-leaves form of the predict exchange: zeros in, the total out
        tot = m.ctx.aggregate_exchange_empty(3, Xt.shape[0])
        assert tot.shape == (3, Xt.shape[0]) and np.all(tot == 0.0)
        m.ctx.comm_destroy()


def test_config5_full_size_factor_and_discard():
    """BASELINE config 5 at its REAL size (VERDICT r2 #3a): buildDSMGP K=4 splits V=3 M=500 N=500k D=16 with
    KernelFunction[IsoSE, IsoLinear], depth 2 -> 288 leaf GPs, n = 7.7k..83k (a 55 GB factor; npad^2 far past int32),
    2.8 TB of factors streamed through one 288 GB GPU in ~12 leaf groups (factor-and-discard, one device pool), the 50k test
    rows riding through every group.  Too large for the oracle: checked through size-independent properties -- info == 0 and
    finite log-marginals everywhere, finite positive predictions, the residual of K_y alpha = y - m on the LARGEST leaf of
    each kernel (rows of K_y assembled on the host; alpha fetched before the leaf's group is discarded), and
    streamed == resident on two mid-size leaves refitted in a plain context.  About two minutes of GPU time."""
    N, D = 500_000, 16
    X, y, Xt = regression_data(N, D, seed=20205)
    kern = [dsm.IsoSE(np.log(0.3), 0.0), dsm.IsoLinear(np.log(1.5))]
    m = dsm.buildDSMGP(X, y, 3, 4, M=500, D=2, kernel=kern, logNoise=np.log(0.1), seed=20205, fit_now=False,
                       stream_budget="auto")
    nobs = np.array([lf.nobs for lf in m.leaves])
    kind = np.array([lf.kernel.kind for lf in m.leaves])
    assert m.L == 288 and nobs.max() > 80_000 and float(np.sum(nobs.astype(float) ** 2)) * 8 > 2.5e12
    big = [int(np.flatnonzero(kind == k)[np.argmax(nobs[kind == k])]) for k in (0, 2)]
    m.ctx.keep_alpha = tuple(big)
    dsm.resident_test(m, Xt)
    dsm.fit(m)
    assert isinstance(m.ctx, hipabi.StreamingContext) and len(m.ctx.groups) >= 8
    assert np.all(m.leaf_info == 0) and np.all(np.isfinite(m.leaf_mll))
    z = dsm.infer(m)
    passes = m.ctx.passes
    mu, var = dsm.predict(m, Xt)
    assert m.ctx.passes == passes                          # the test rows rode through the fit pass
    assert np.isfinite(z) and np.all(np.isfinite(mu)) and np.all(var > 0)
    rng = np.random.default_rng(5)
    for j in big:                                           # K_y alpha = y - m on 4096 sampled rows + the first and last 64
        lf = m.leaves[j]
        alpha = m.ctx.alpha(j)
        xs, yc = X[lf.obs], y[lf.obs] - lf.mean.m
        c = np.exp(2 * lf.logNoise) + 1e-8
        rows = np.unique(np.concatenate([np.arange(64), np.arange(lf.nobs - 64, lf.nobs), rng.choice(lf.nobs, 4096, replace=False)]))
        if lf.kernel.kind == 2:
            r = xs[rows] @ (xs.T @ alpha) / np.exp(2 * lf.kernel.logl)
        else:
            l2, s2 = np.exp(2 * lf.kernel.logl), np.exp(2 * lf.kernel.logs)
            sq = np.sum(xs * xs, axis=1)
            r = np.empty(rows.size)
            for a in range(0, rows.size, 512):
                rr = rows[a:a + 512]
                P = np.maximum(sq[rr, None] + sq[None, :] - 2.0 * (xs[rr] @ xs.T), 0.0)
                r[a:a + 512] = (s2 * np.exp(-0.5 * P / l2)) @ alpha
        r += c * alpha[rows] - yc[rows]
        assert np.max(np.abs(r)) <= 1e-7 * np.max(np.abs(yc)), (lf.nobs, lf.kernel.kind, float(np.max(np.abs(r))))
    order = np.argsort(nobs)
    mid = [int(j) for j in order[143:145]]
    c2 = hipabi.Context(0)
    c2.set_train(X, y)
    lv = [m.leaves[j] for j in mid]
    c2.set_leaves(np.concatenate([[0], np.cumsum([lf.nobs for lf in lv])]), np.concatenate([lf.obs for lf in lv]),
                  [lf.kernelid for lf in lv], [lf.mean.m for lf in lv])
    for lf in m.kernel_table():
        c2.set_hyper(lf.kernelid, lf.kernel.kind, np.concatenate([lf.kernel.loghyp(), [lf.logNoise]]))
    mll2, info2, _ = c2.fit()
    c2.close()
    assert np.all(info2 == 0) and np.allclose(mll2, m.leaf_mll[mid], rtol=1e-10)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_diagonal_blocks_one_step_ahead_agree_with_separate_launches(ctx, kind):
    """Round 4 (shorten the chain).  Two schedules of the block steps that are not fused:
      classic   update / reduce / diagonal block / panel solve launches (DSMGP_OPT_DIAG_IN_UPDATE off);
      ahead     the default: the update launch of step k - 1 also updates tile (k, k) over its columns, the update launch of
                step k carries one task per leaf that applies the last block column, factorises and inverts -- no
                diagonal-block launch on the chain.
    Thirteen leaves of 200..4100 rows (33 block steps: launches with fewer tiles than CUs, where every tile is split along K,
    and fuller ones) with a COPY and a PREFIX leaf and routed test rows, every step on the schedule under test and then the
    default mix with the fused shallow steps, against `classic`: log-marginals 1e-12, factors 1e-11, moments 1e-9; two
    leaves against the oracle; the same fit three times gives the same bits; and the paths that need the WHOLE inverse of
    the fused steps' diagonal blocks afterwards (alpha, standalone prediction) agree too."""
    N, D, L = 20_000, 3, 13
    X, y, Xt = regression_data(N, D, n_test=200, seed=6300 + kind)
    rng = np.random.default_rng(31 + kind)
    sizes = [200, 333, 512, 640, 777, 900, 1100, 1290, 1500, 1900, 333, 700, 4100]
    obs = [np.sort(rng.choice(N, size=int(n), replace=False)) for n in sizes]
    obs[10] = obs[1].copy()                                               # COPY of leaf 1
    tail = np.arange(obs[3][-1] + 1, min(N, obs[3][-1] + 1 + 200))
    obs[11] = np.concatenate([obs[3], tail])                              # leaf 3 is a strict prefix of leaf 11
    op = np.zeros(L, dtype=np.int32)
    src = np.full(L, -1, dtype=np.int32)
    plen = np.zeros(L, dtype=np.int64)
    op[10], src[10] = 1, 1
    if tail.size:
        op[11], src[11], plen[11] = 2, 3, obs[3].size
    ntest = rng.integers(20, 180, size=L)
    rptr = np.concatenate([[0], np.cumsum(ntest)])
    ridx = np.concatenate([np.sort(rng.choice(Xt.shape[0], size=int(k), replace=False)) for k in ntest])
    hyp = {0: [np.log(0.3), 0.0, np.log(0.1)], 1: [np.log(0.3), np.log(0.4), np.log(0.5), 0.0, np.log(0.1)],
           2: [np.log(1.5), 0.0, np.log(0.3)]}[kind]
    means = [float(np.mean(y[o])) for o in obs]
    means[10] = means[1]
    schedules = {"classic": 0, "ahead": 1}

    def run(schedule, fused_steps):
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1 if fused_steps else 0)
        ctx.set_option(hipabi.OPT_DIAG_IN_UPDATE, schedules[schedule])
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, dtype=np.int32), means)
        ctx.set_sharing(op, src, plen)
        ctx.set_hyper(0, kind, hyp)
        ctx.set_test(Xt, rptr, ridx)
        mll, info, _ = ctx.fit()
        assert np.all(info == 0)
        ctx.predict_run()
        mu, var = ctx.predict_fetch()
        fa = [ctx.download_factor(j, obs[j].size) for j in (0, 9, 10, 11, 12)]
        for _ in range(2):                           # again: same launches, same order of arithmetic
            mll2, _, _ = ctx.fit()
            ctx.predict_run()
            mu2, var2 = ctx.predict_fetch()
            assert np.array_equal(mll, mll2) and np.array_equal(mu, mu2) and np.array_equal(var, var2)
        ctx.set_joint(False)                         # the drop-in call pattern: fit without the rows, then the standalone sweep
        ctx.fit()
        ctx.predict_run()
        mu3, var3 = ctx.predict_fetch()
        ctx.set_joint(True)
        assert np.allclose(mu3, mu, rtol=1e-9, atol=1e-11) and np.allclose(var3, var, rtol=1e-8, atol=1e-12)
        return mll, mu, var, fa

    try:
        runs = [(run("ahead", fs), run("classic", fs), "ahead", fs) for fs in (False, True)]
    finally:
        ctx.set_option(hipabi.OPT_DIAG_IN_UPDATE, 1)
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
    for a, b, sch, fs in runs:
        assert np.allclose(a[0], b[0], rtol=1e-12, atol=0), (sch, fs, float(np.max(np.abs(a[0] - b[0]) / np.abs(b[0]))))
        emu = float(np.max(np.abs(a[1] - b[1])) / max(1.0, float(np.max(np.abs(b[1])))))
        evar = float(np.max(np.abs(a[2] - b[2]) / np.abs(b[2])))
        assert emu <= 1e-9 and evar <= 1e-9, (sch, fs, emu, evar)
        for (Fa, aa), (Fb, ab) in zip(a[3], b[3]):
            assert np.max(np.abs(Fa - Fb)) <= 1e-11 * np.max(np.abs(Fb)), (sch, fs, float(np.max(np.abs(Fa - Fb)) / np.max(np.abs(Fb))))
            assert np.max(np.abs(aa - ab)) <= 1e-8 * np.max(np.abs(ab)), (sch, fs)
    a = runs[1][0]                                   # the default: diagonal blocks ahead, behind the fused shallow steps
    mk = {0: lambda: ogp.IsoSE(hyp[0], hyp[1]), 1: lambda: ogp.ArdSE(np.array(hyp[:3]), hyp[3]), 2: lambda: ogp.IsoLinear(hyp[0])}[kind]
    for j in (11, 12):
        g = ogp.GaussianProcess(X[obs[j]], y[obs[j]], means[j], mk(), hyp[-1], True).update_cholesky()
        assert abs(a[0][j] - g.mll()) <= RTOL * abs(g.mll())
        mo, vo = g.prediction(Xt[ridx[rptr[j]:rptr[j + 1]]])
        assert np.allclose(a[1][rptr[j]:rptr[j + 1]], mo, rtol=RTOL, atol=1e-9)
        assert np.allclose(a[2][rptr[j]:rptr[j + 1]], vo, rtol=RTOL, atol=1e-10)


def test_fit_replayed_as_a_graph_equals_plain_launches(ctx):
    """DSMGP_OPT_FIT_GRAPH (round 4; opt-in): with per-launch timing off dsmgp_fit replays its launch sequence as
    a captured hipGraph.  Same kernels and arguments: the results equal those of plain launches BIT FOR BIT -- also after the
    hyper-parameters change (they travel through the CONTENTS of the kernel-parameter table, which the graph only points at),
    with and without resident test rows, with a COPY and a PREFIX leaf (the graph holds the device-to-device copies of the
    prefix blocks), and after a new leaf table (the old graphs are dropped with their plan)."""
    N, D, L = 8000, 3, 6
    X, y, Xt = regression_data(N, D, n_test=120, seed=1234)
    rng = np.random.default_rng(9)
    sizes = [300, 700, 1500, 400, 700, 900]
    obs = [np.sort(rng.choice(N, size=n, replace=False)) for n in sizes]
    obs[4] = obs[1].copy()
    tail = np.arange(obs[3][-1] + 1, min(N, obs[3][-1] + 401))
    obs[5] = np.concatenate([obs[3], tail])
    op = np.array([0, 0, 0, 0, 1, 2], dtype=np.int32)
    src = np.array([-1, -1, -1, -1, 1, 3], dtype=np.int32)
    plen = np.array([0, 0, 0, 0, 0, obs[3].size], dtype=np.int64)
    means = [float(np.mean(y[o])) for o in obs]
    means[4] = means[1]
    ntest = rng.integers(10, 100, size=L)
    rptr = np.concatenate([[0], np.cumsum(ntest)])
    ridx = np.concatenate([np.sort(rng.choice(Xt.shape[0], size=int(k), replace=False)) for k in ntest])
    hypers = [[np.log(0.3), 0.0, np.log(0.1)], [np.log(0.5), 0.2, np.log(0.2)], [np.log(0.3), 0.0, np.log(0.1)]]

    def run(graph):
        ctx.set_option(hipabi.OPT_FIT_GRAPH, 1 if graph else 0)
        ctx.set_profile(0)
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, dtype=np.int32), means)
        ctx.set_sharing(op, src, plen)
        out = []
        for h in hypers:                              # fit alone: the graph of the plain step lists
            ctx.set_hyper(0, 0, h)
            mll, info, _ = ctx.fit()
            assert np.all(info == 0)
            out.append(mll)
        ctx.set_test(Xt, rptr, ridx)
        for h in hypers[:2]:                          # with the rows riding along: the second graph
            ctx.set_hyper(0, 0, h)
            mll, info, _ = ctx.fit()
            ctx.predict_run()
            mu, var = ctx.predict_fetch()
            out += [mll, mu, var]
        out.append(ctx.download_factor(5, obs[5].size)[0])
        return out

    try:
        a, b = run(True), run(False)
    finally:
        ctx.set_option(hipabi.OPT_FIT_GRAPH, 0)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert not np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2])     # the replay follows the hyper-parameters


@pytest.mark.parametrize("order", ["none", "import", "first"])
def test_rccl_communicator_comes_up_in_every_import_order(order):
    """A PyTorch wheel bundles its own ROCm runtime; a process holds one or two runtimes depending on who came first, and
    the library's RCCL loader must pick the librccl of the runtime the library is bound to.  Child processes:
    no torch at all; the library first and torch imported afterwards (two runtimes: the system's owns the GPU, RCCL must be
    the system's); torch.cuda first (the order of every torch.distributed job: the library binds to torch's runtime by
    SONAME, ONE libamdhip64 in the process, torch keeps working)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "diag_rccl_maps.py"), order], capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "comm_init ok: [[0. 1. 2.]]" in r.stdout, r.stdout[-2000:]
    end = [ln for ln in r.stdout.splitlines() if ln.startswith("at the end:")][-1]
    if order == "first":
        assert "torch still works: 8.0" in r.stdout
        assert end.count("libamdhip64") == 1 and "/opt/rocm" not in end, end
    elif order == "none":
        assert "torch/lib" not in end


def test_test_set_replaced_between_a_joint_fit_and_its_first_use(ctx):
    """Round-4 advisor (high): a fit with its test rows riding along leaves the diagonal blocks of the fused steps with their
    16x16 diagonal inverses only; the rest of Dinv_k is completed on first use (ensure_dinv) from a task list that used to
    belong to the TEST set's step lists -- so `fit; predict(Xval); ...; fit; predict(Xnew)` (set_test, joint fit, set_test of
    other rows, then the standalone sweep or the gradients) launched the completion over a freed list.  The list is the
    plan's now.  40 leaves (>= 32: the shallow steps run fused), checked per leaf against the oracle."""
    N, D, L = 40 * 330, 2, 40
    X, y, Xa = regression_data(N, D, n_test=64, seed=515)
    _, _, Xb = regression_data(N, D, n_test=48, seed=516)
    sizes = 200 + (np.arange(L) * 37) % 130
    obs_ptr = np.concatenate([[0], np.cumsum(sizes)])
    obs = [np.arange(330 * l, 330 * l + sizes[l]) for l in range(L)]
    means = [float(np.mean(y[o])) for o in obs]
    h = np.array([np.log(0.35), 0.1, np.log(0.15)])
    ctx.set_train(X, y)
    ctx.set_leaves(obs_ptr, np.concatenate(obs), np.zeros(L, np.int32), means)
    ctx.set_hyper(0, 0, h)
    ctx.set_joint(True)
    ra = (np.arange(L + 1) * Xa.shape[0], np.tile(np.arange(Xa.shape[0]), L))
    rb = (np.arange(L + 1) * Xb.shape[0], np.tile(np.arange(Xb.shape[0]), L))
    gps = [ogp.GaussianProcess(X[o], y[o], m, ogp.make_kernel(0, h[:2]), h[2], True).update_cholesky() for o, m in zip(obs, means)]

    def check_prediction(Xt):
        mu, var = ctx.predict_fetch()
        for l, g in enumerate(gps):
            mo, vo = g.prediction(Xt)
            sl = slice(l * Xt.shape[0], (l + 1) * Xt.shape[0])
            assert np.allclose(mu[sl], mo, rtol=RTOL, atol=1e-10) and np.allclose(var[sl], vo, rtol=RTOL, atol=1e-10), l

    ctx.set_test(Xa, *ra)
    ctx.fit()                                   # joint: rows of Xa ride along, Dinv_k of the fused steps stays incomplete
    ctx.set_test(Xb, *rb)                       # frees the joint step lists
    ctx.predict_run()                           # standalone sweep: needs the whole Dinv_k
    check_prediction(Xb)
    ctx.set_test(Xa, *ra)
    ctx.fit()
    ctx.set_test(Xb, *rb)
    g = ctx.gradients(3)                        # ... and so do the gradients (L^-T from Dinv_k) and alpha
    for l, gp_ in enumerate(gps):
        go = gp_.grad()
        assert np.max(np.abs(g[l] - go)) <= 1e-7 * max(1.0, float(np.max(np.abs(go)))), (l, g[l], go)
    ctx.predict_run()
    check_prediction(Xb)


def test_device_routing_equals_the_host_routing_entry_by_entry():
    """predict(model, x) on rows the model has not seen routes them on the device (dsmgp_set_tree + dsmgp_set_test_routed:
    `src/common.jl:101-122,181-196,275-292` as one thread per row, the walk of csrc/route_walk.hpp that the host routine
    dsmgp_tree_route runs too).  The CSR it leaves in HBM must be the host routine's, entry by entry -- complete and ragged
    trees, kernel vectors, one input dimension, rows exactly ON thresholds, +-Inf coordinates -- and the prediction built on it
    must equal, to the bit, the prediction of the host-routed registration (same entry index, same summation order).
    A row outside every region (NaN) is refused; a shard that holds half of the leaves gets exactly its half."""
    cases = [dict(N=3000, D=3, K=3, V=4, M=40, depth=3), dict(N=700, D=2, K=2, V=3, M=60, depth=4),
             dict(N=500, D=1, K=3, V=4, M=10, depth=2), dict(N=2000, D=5, K=1, V=5, M=100, depth=2)]
    for i, c in enumerate(cases):
        X, y, Xt = regression_data(c["N"], c["D"], n_test=333, seed=900 + i)
        kern = [dsm.IsoSE(np.log(0.4), 0.0), dsm.IsoLinear(0.0)] if i == 0 else dsm.IsoSE(np.log(0.4), 0.0)
        m = dsm.buildDSMGP(X, y, c["K"], c["V"], M=c["M"], D=c["depth"], kernel=kern, logNoise=np.log(0.2), seed=40 + i)
        assert m._device_routing
        node = m.root.children[0] if m.root.kind == "sum" else m.root
        d = node.split[0][0]
        on = np.repeat(Xt[:1], len(node.split) - 1, axis=0)
        on[:, d] = [t for (_, t) in node.split[:-1]]                       # rows ON the thresholds: the child on the low side
        inf = Xt[:2].copy()
        inf[0, d], inf[1, d] = -np.inf, np.inf                             # the first child has no lower test, the last bound is +Inf
        for xt in (Xt, np.vstack([Xt[:50], on, inf]), Xt[:1]):
            hp, hi = ptree.route(m.root, xt)
            dp = m.ctx.set_test_routed(xt)
            gp_, gi = m.ctx.routes()
            assert np.array_equal(dp, hp) and np.array_equal(gp_, hp) and np.array_equal(gi, hi)
        dsm.update(m)
        mu_d, var_d = dsm.predict(m, Xt)
        m._device_routing, m._route_cache = False, None
        mu_h, var_h = dsm.predict(m, Xt)
        assert np.array_equal(mu_d, mu_h) and np.array_equal(var_d, var_h)
        m._device_routing, m._route_cache = True, None
        bad = Xt[:5].copy()
        bad[3, d] = np.nan
        with pytest.raises(hipabi.DsmgpError) as e:
            dsm.predict(m, bad)
        assert "outside" in str(e.value)
        mu_again, _ = dsm.predict(m, Xt)                                   # the refused registration left nothing behind
        assert np.array_equal(mu_again, mu_d)
    # half of the leaves (what one of two ranks holds): regions of the other half carry -1 and are skipped
    ri = ptree.route_index(m.root)
    loc = np.arange(0, m.L, 2)
    lv = [m.leaves[j] for j in loc]
    ptr, idx = ptree.obs_table(lv)
    c2 = hipabi.Context(0)
    c2.set_train(X, y)
    c2.set_leaves(ptr, idx, [lf.kernelid for lf in lv], [lf.mean.m for lf in lv])
    g2l = np.full(m.L, -1, dtype=np.int64)
    g2l[loc] = np.arange(loc.size)
    c2.set_tree(ri.kind, ri.first, ri.nchild, ri.sdim, ri.thr, np.where(ri.leaf >= 0, g2l[np.maximum(ri.leaf, 0)], -1))
    c2.set_test_routed(Xt)
    p2, i2 = c2.routes()
    hp, hi = ptree.route(m.root, Xt)
    assert np.array_equal(np.diff(p2), np.diff(hp)[loc])
    assert np.array_equal(i2, np.concatenate([hi[hp[j]:hp[j + 1]] for j in loc]))
    with pytest.raises(hipabi.DsmgpError):                                 # a region naming a leaf beyond the table
        c2.set_tree(ri.kind, ri.first, ri.nchild, ri.sdim, ri.thr, np.where(ri.leaf >= 0, ri.leaf, -1))
    c2.set_leaves(ptr, idx, [lf.kernelid for lf in lv], [lf.mean.m for lf in lv])   # a new leaf table drops the tree
    with pytest.raises(hipabi.DsmgpError) as e:
        c2.set_test_routed(Xt)
    assert "set_tree" in str(e.value)
    c2.close()


def test_two_leaf_lanes_agree_with_one_lane(ctx):
    """DSMGP_OPT_LANES (round 5): the leaves of a table dealt into two halves with step lists, split-K workspace and stream of their
    own, joined at the end of fit! (`src/fit.jl:88-119`: the leaves are independent).  (1) A table whose block steps all run fused
    -- 300 leaves of 130..640 rows: no split-K anywhere -- gives the one-lane schedule's results to the BIT, per leaf: log-marginals,
    moments of routed rows riding through the fit and of the standalone sweep, gradients.  (2) A table of few large leaves
    (classic steps: a launch of half the tiles cuts its tail along K differently) agrees to rounding, 1e-12 / 1e-10, and against
    the oracle on sampled leaves at the north-star tolerance.  (3) Two fits with two lanes are bit-identical (fixed summation
    orders per lane, no atomics); the automatic rule takes two lanes from 8 sharing groups on and one below."""
    def table(sizes, seed, D=3, n_test=96):
        N = int(np.sum(sizes)) + 10
        X, y, Xt = regression_data(N, D, n_test=n_test, seed=seed)
        rng = np.random.default_rng(seed)
        obs = [np.sort(rng.choice(N, size=int(n), replace=False)) for n in sizes]
        obs[1] = obs[0].copy()                                            # a COPY leaf: rides in its source's lane
        return X, y, Xt, obs

    def run(lanes, X, y, Xt, obs, joint):
        L = len(obs)
        ctx.set_option(hipabi.OPT_LANES, lanes)
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, np.int32),
                       [float(np.mean(y[o])) for o in obs])
        op, src = np.zeros(L, np.int32), np.full(L, -1, np.int32)
        op[1], src[1] = 1, 0
        ctx.set_sharing(op, src, np.zeros(L, np.int64))
        ctx.set_hyper(0, 0, [np.log(0.4), 0.1, np.log(0.15)])
        ctx.set_joint(joint)
        rp = np.arange(L + 1) * Xt.shape[0]
        ri = np.tile(np.arange(Xt.shape[0]), L)
        if joint:
            ctx.set_test(Xt, rp, ri)
        mll, info, _ = ctx.fit()
        assert np.all(info == 0)
        if not joint:
            ctx.set_test(Xt, rp, ri)
        ctx.predict_run()
        mu, var = ctx.predict_fetch()
        return mll, mu, var, ctx.gradients(3), ctx.lanes()

    try:
        # (1) fused steps only
        sizes = np.random.default_rng(5).integers(130, 641, size=300)      # five block steps at most: all of them run fused
        X, y, Xt, obs = table(sizes, 7101)
        for joint in (False, True):
            one, two = run(1, X, y, Xt, obs, joint), run(2, X, y, Xt, obs, joint)
            assert one[4] == 1 and two[4] == 2
            for a, b in zip(one[:4], two[:4]):
                assert np.array_equal(a, b)
        again = run(2, X, y, Xt, obs, True)
        assert all(np.array_equal(a, b) for a, b in zip(two[:4], again[:4]))
        # the captured hipGraph of a two-lane fit (fork / join across the lanes' streams inside the capture) replays the same bits
        ctx.set_option(hipabi.OPT_FIT_GRAPH, 1)
        ctx.set_profile(0)
        try:
            g1 = run(2, X, y, Xt, obs, True)
            g2 = ctx.fit()
            assert all(np.array_equal(a, b) for a, b in zip(two[:4], g1[:4])) and np.array_equal(g2[0], two[0])
            four = run(4, X, y, Xt, obs, True)
            assert four[4] == 4 and all(np.array_equal(a, b) for a, b in zip(two[:4], four[:4]))
        finally:
            ctx.set_option(hipabi.OPT_FIT_GRAPH, 0)
        assert run(0, X, y, Xt, obs, True)[4] == 2                         # automatic: 299 sharing groups
        # (2) classic steps, split along K
        sizes = np.array([2100, 2100, 1900, 1700, 1500, 1300, 900, 700, 2300, 1100])
        X, y, Xt, obs = table(sizes, 7102, n_test=150)
        one, two = run(1, X, y, Xt, obs, True), run(2, X, y, Xt, obs, True)
        assert two[4] == 2 and run(0, X, y, Xt, obs, True)[4] == 2         # automatic: 9 sharing groups -> two lanes
        few = [o for o in obs[:5]]
        assert run(0, X, y, Xt, few, True)[4] == 1                         # 4 sharing groups -> one
        assert np.allclose(one[0], two[0], rtol=1e-12) and np.allclose(one[1], two[1], rtol=1e-10, atol=1e-12)
        assert np.allclose(one[2], two[2], rtol=1e-9, atol=1e-13) and np.allclose(one[3], two[3], rtol=1e-8, atol=1e-9)
        for l in (0, 7, 8):
            g = ogp.GaussianProcess(X[obs[l]], y[obs[l]], float(np.mean(y[obs[l]])), ogp.make_kernel(0, [np.log(0.4), 0.1]), np.log(0.15),
                                    True).update_cholesky()
            mo, vo = g.prediction(Xt)
            sl = slice(l * Xt.shape[0], (l + 1) * Xt.shape[0])
            assert abs(two[0][l] - g.mll()) <= RTOL * abs(g.mll())
            assert np.allclose(two[1][sl], mo, rtol=RTOL, atol=1e-10) and np.allclose(two[2][sl], vo, rtol=RTOL, atol=1e-10)
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)
        ctx.set_joint(True)


# ------------------------------------------------------------------------------------ round 6

def test_test_matrix_width_travels_through_the_abi(ctx):
    """dsmgp_set_test / dsmgp_set_test_routed / dsmgp_predict_leaves take the caller's D and return
    DSMGP_E_ARG on a mismatch (they read n_t * D doubles from the caller's buffer); the Python context refuses before the call."""
    import ctypes as C
    X, y, Xt = regression_data(300, 3, n_test=20, seed=61)
    _single(ctx, X, y, 0.0, 0, np.array([np.log(0.5), 0.0]), np.log(0.2))
    ptr = np.array([0, 20], dtype=np.int64)
    idx = np.arange(20, dtype=np.int64)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    xt = np.asfortranarray(Xt)
    for D_claimed, want in ((2, hipabi.E_ARG), (4, hipabi.E_ARG), (3, 0)):
        rc = ctx.lib.dsmgp_set_test(ctx.h, xt.ctypes.data_as(dp), 20, D_claimed, ptr.ctypes.data_as(lp), idx.ctypes.data_as(lp))
        assert rc == want, (D_claimed, rc)
    assert "columns" in ctx.lib.dsmgp_last_error(ctx.h).decode() or True
    ctx.set_tree(np.zeros(1, dtype=np.int8), [0], [0], [0], np.zeros((1, 1)), [0])
    assert ctx.lib.dsmgp_set_test_routed(ctx.h, xt.ctypes.data_as(dp), 20, 2) == hipabi.E_ARG
    assert "columns" in ctx.lib.dsmgp_last_error(ctx.h).decode()
    assert ctx.lib.dsmgp_set_test_routed(ctx.h, xt.ctypes.data_as(dp), 20, 3) == 0
    mu = np.empty(20)
    var = np.empty(20)
    assert ctx.lib.dsmgp_predict_leaves(ctx.h, xt.ctypes.data_as(dp), 20, 5, ptr.ctypes.data_as(lp), idx.ctypes.data_as(lp),
                                        mu.ctypes.data_as(dp), var.ctypes.data_as(dp)) == hipabi.E_ARG
    with pytest.raises(ValueError, match="D = 3"):
        ctx.set_test(Xt[:, :2], ptr, idx)
    with pytest.raises(ValueError, match="D = 3"):
        ctx.set_test_routed(Xt[:, :2])
    mu1, var1 = ctx.predict_leaves(Xt, ptr, idx)                       # the context is still usable, and right
    g = ogp.GaussianProcess(X, y, 0.0, ogp.make_kernel(0, [np.log(0.5), 0.0]), np.log(0.2)).update_cholesky()
    mo, vo = g.prediction(Xt)
    assert np.allclose(mu1, mo, rtol=RTOL, atol=1e-10) and np.allclose(var1, vo, rtol=RTOL, atol=1e-10)


def test_outside_row_is_the_same_error_on_the_device_and_on_the_host_path():
    """a row outside a split region raised DsmgpError on the device path and ValueError on the host path.  Now
    DSMGP_E_DOMAIN -> DsmgpDomainError, which IS a ValueError; the model stays usable."""
    X, y, Xt = regression_data(1500, 2, n_test=50, seed=62)
    m = dsm.buildDSMGP(X, y, 2, 3, M=60, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), seed=4)
    mu, var = dsm.predict(m, Xt)
    d = m.root.children[0].split[0][0]
    bad = Xt[:6].copy()
    bad[2, d] = np.nan
    for routing in (True, False):
        m._device_routing, m._route_cache = routing, None
        with pytest.raises(ValueError, match="outside"):
            dsm.predict(m, bad)
    m._device_routing, m._route_cache = True, None
    mu2, var2 = dsm.predict(m, Xt)
    assert np.array_equal(mu, mu2) and np.array_equal(var, var2)


def test_registration_does_not_depend_on_what_the_arena_held_before():
    """the K_tn arena is no longer cleared at registration; correctness rests on no kernel reading padding rows a
    previous test set left behind.  Poison it: a first, LARGER test set whose rows carry NaN in a dimension the tree never
    splits on (a PoE tree cuts dimension 0 only, src/treeStructure.jl:190) fills every routed row of the arena with NaN; the
    second, smaller set must then predict, bit for bit, what a context that never saw the poison predicts."""
    X, y, Xt = regression_data(2600, 3, n_test=700, seed=63)
    kw = dict(M=150, kernel=dsm.IsoSE(np.log(0.4), 0.0), meanFun=dsm.ConstMean(0.0), logNoise=np.log(0.2), seed=5)
    clean = dsm.buildPoE(X, y, 4, **kw)
    Xs = Xt[:157]                                                     # ragged: not a multiple of any tile size
    mu0, var0 = dsm.predict(clean, Xs)
    for joint in (False, True):
        m = dsm.buildPoE(X, y, 4, **kw)
        poison = Xt.copy()
        poison[:, 1] = np.nan
        mu_p, _ = dsm.predict(m, poison)
        assert np.all(np.isnan(mu_p))                                  # the arena now holds NaN wherever a row was routed
        if joint:                                                      # ... and once more through the joint fit (rows riding along)
            dsm.fit(m)
            dsm.predict(m, poison)
        mu1, var1 = dsm.predict(m, Xs)
        assert np.array_equal(mu1, mu0) and np.array_equal(var1, var0), joint
        if joint:
            dsm.fit(m)                                                 # the small set rides through a fit over the poisoned arena
            mu2, var2 = dsm.predict(m, Xs)
            assert np.allclose(mu2, mu0, rtol=1e-12, atol=1e-14) and np.allclose(var2, var0, rtol=1e-12, atol=1e-14)
            assert np.all(np.isfinite(mu2)) and np.all(np.isfinite(var2))


def test_native_tree_builder_equals_the_oracle_restatement_at_bench_sizes():
    """SURVEY 8(f).1 / VERDICT r5 #5 on the GPU box's host: the table dsmgp_tree_build exports for the BENCH models -- config 1
    at full size, the headline model (N = 100k, depth 2) at full size, depth 4 at N = 30k, configs 3 and 5 at reduced N --
    against oracle/tree.py, bit for bit (kinds, thresholds, obs CSR, means, Dirichlet draws)."""
    from test_host_cpu import _native_table_equals_oracle, TREE_ORACLE_CASES
    for (N, D, M, K, V, depth, eps, sr, nk, seed) in TREE_ORACLE_CASES + [(100_000, 8, 200, 4, 3, 2, 0.5, True, 0, 20204),
                                                                          (30_000, 8, 200, 4, 3, 4, 0.5, True, 0, 20204)]:
        X, y, _ = regression_data(N, D, seed=20204 if N >= 30_000 else 20200 + D)
        nodes, regions = _native_table_equals_oracle(X, y, M, K, V, depth, eps, sr, nk, seed)
        if N == 100_000:
            assert regions == 144                                      # the 144 leaves of the headline bench line


def test_predict_with_unnormalised_weights_on_the_device_moments():
    """src/common.jl:134-143,275-302: hand-assigned sum-node weights that do not add up to one leave (mu_min - 1)(1 - sum w) in
    the mean; the product then runs the literal recursion on the per-(leaf, row) moments of the device (model.predict)."""
    X, y, Xt = regression_data(1200, 2, n_test=80, seed=64)
    m = dsm.buildDSMGP(X, y, 3, 3, M=50, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), seed=9)
    dsm.update(m)
    gps = ospn.make_leaf_gps(m.root, X, y, exact_dist=True)
    ospn.fit(m.root, gps, ospn.get_overlap(m.root, m.L))
    mu_n, var_n = dsm.predict(m, Xt)
    m.root.logweights = np.log(np.array([0.6, 0.3, 0.3]))
    mu_u, var_u = dsm.predict(m, Xt)
    mo, vo = ospn.predict(m.root, gps, Xt)
    assert np.allclose(mu_u, mo, rtol=RTOL, atol=1e-10) and np.allclose(var_u, vo, rtol=RTOL, atol=1e-10)
    assert np.max(np.abs(mu_u - mu_n)) > 1e-3
    dsm.update(m)                                                       # back to the posterior weights: the device aggregation again
    mu_b, var_b = dsm.predict(m, Xt)
    assert np.array_equal(mu_b, mu_n) and np.array_equal(var_b, var_n)


def test_duplicate_training_points_and_test_points_on_training_points(ctx):
    """Collisions as the domain has them: exact duplicates among the training rows (K singular, K + noise I not) and test rows that
    ARE training rows (the smallest predictive variances the model can give), for the three kernel kinds, against the oracle."""
    D = 3
    base = uniform(70, 0, 150 * D).reshape((150, D), order="F")
    X = np.asfortranarray(np.vstack([base, base[:90], base[:40]]))                  # 280 rows, 130 of them copies
    y = np.sin(4 * X[:, 0]) + 0.05 * normal(71, 0, X.shape[0])
    Xt = np.asfortranarray(np.vstack([base[:25], uniform(72, 0, 20 * D).reshape((20, D), order="F")]))
    for kind, h in ((0, [np.log(0.4), 0.1]), (1, list(np.log([0.3, 0.6, 0.9])) + [0.0]), (2, [np.log(1.3), 0.0])):
        logn = np.log(0.15)
        mll, info, _ = _single(ctx, X, y, 0.1, kind, np.array(h), logn)
        assert info[0] == 0
        g = ogp.GaussianProcess(X, y, 0.1, ogp.make_kernel(kind, h), logn, exact_dist=True).update_cholesky()
        assert abs(mll[0] - g.mll()) <= RTOL * abs(g.mll()), kind
        n_t = Xt.shape[0]
        mu, var = ctx.predict_leaves(Xt, np.array([0, n_t]), np.arange(n_t))
        mo, vo = g.prediction(Xt)
        assert np.allclose(mu, mo, rtol=RTOL, atol=1e-10), kind
        assert np.allclose(var, vo, rtol=RTOL, atol=1e-12) and np.all(var > 0), kind


def test_bench_two_ranks_over_gloo_prints_one_json_line():
    """bench.py --gpus 2 without a launcher (it starts its own two ranks under torch.distributed.run), exchange over gloo with both
    ranks on this one GPU: the rehearsal of the N > 1 bench path the driver runs on a multi-GPU node.  Rank 0's stdout must carry
    ONE JSON line and nothing else (gloo announces its connections on stdout: bench.py points fd 1 at stderr while the groups come
    up), with both ranks' shares, the exchange seconds, and no device-exchange series (that needs RCCL and --full)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DSMGP_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline",
                        "--config", "dsmgp_n20k_d8"], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:500]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["exchange_backend"] == "gloo" and d["device_exchange_series"] is None
    assert d["scaling"] == "strong" and d["unit"] == "s" and d["value"] > 0
    ranks = d["ranks"]
    assert [x["rank"] for x in ranks] == [0, 1] and sum(x["n_leaves"] for x in ranks) == 144
    assert abs(sum(x["cholesky_flop_share"] for x in ranks) - 1.0) < 1e-12
    assert all(x["exchanges_per_step"] == 2 and x["exchange_s_per_step"] > 0 for x in ranks)


def test_bench_plain_line_leaves_the_extras_to_full(tmp_path):
    """A plain `bench.py --gpus 1` run does only what its headline figure needs: the line carries the headline keys, the per-step
    spread and the roofline of the timed launches, and none of what --full adds (probe, drop-in series, one-lane step, other
    configs, CPU baseline); --dump-outputs still writes the last timed step, whose root log-marginal is the line's."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--config", "dsmgp_n20k_d8", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[:500]
    j = json.loads(lines[0])
    assert j["unit"] == "s" and j["higher_is_better"] is False and j["dtype"] == "f64" and j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and abs(j["ms_per_step"] - 1e3 * j["value"]) <= 1e-9 * j["ms_per_step"]
    assert j["step_s"]["min"] <= j["step_s"]["median"] <= j["step_s"]["max"] and j["roofline"]["bound"] == "mfma"
    assert not {"f64_mfma_probe", "drop_in", "drop_in_s", "configs", "cpu_baseline"} & set(j)
    assert not {"frac_of_probe", "single_lane"} & set(j["roofline"]) and 1.0 < j["roofline"]["clock_ghz_in_steps"] < 3.0
    d = {k: np.load(tmp_path / f"{k}.npy") for k in ("mu", "var", "root_mll", "leaf_mll")}
    assert d["root_mll"][0] == j["root_mll"] and d["mu"].shape == d["var"].shape == (2000,) and np.all(d["var"] > 0)
