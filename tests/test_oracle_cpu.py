"""CPU suite, part 1: the oracle against its pins (closed forms, mpmath golden vectors,
finite differences, LAPACK identities).  No GPU."""
import json
import os

import numpy as np
import pytest
import scipy.linalg as sla

from oracle import gp as ogp, spn as ospn
from deepstructuredmixtures_amd.datagen import uniform, normal


def _load_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "gp_small.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    return cases


def test_analytic_n1_n2(golden_dir):
    a = json.load(open(os.path.join(golden_dir, "analytic.json")))
    for name in ("n1", "n2"):
        c = a[name]
        X = np.atleast_1d(np.array(c["x"], dtype=float)).reshape(-1, 1)
        y = np.atleast_1d(np.array(c["y"], dtype=float))
        for exact in (True, False):
            g = ogp.GaussianProcess(X, y, c["mean"], ogp.IsoSE(c["logl"], c["logs"]), c["logNoise"], exact).update_cholesky()
            assert np.allclose(g.alpha, np.atleast_1d(c["alpha"]), rtol=1e-13, atol=0)
            assert abs(g.mll() - c["mll"]) < 1e-13 * abs(c["mll"]) + 1e-14
            mu, var = g.prediction(np.array([[c["xt"]]]))
            assert abs(mu[0] - c["mu"]) < 1e-14 + 1e-13 * abs(c["mu"])
            assert abs(var[0] - c["var"]) < 1e-13
            mu2, S = g.prediction(np.array([[c["xt"]]]), full_cov=True)
            assert abs(S[0, 0] - var[0]) < 1e-14 and mu2[0] == mu[0]


def test_oracle_matches_mpmath_golden(golden_dir):
    for name, c in _load_cases(golden_dir).items():
        k = ogp.make_kernel(int(c["kind"]), c["loghyp"])
        for exact, tol in ((True, 1e-10), (False, 1e-8)):
            g = ogp.GaussianProcess(c["X"], c["y"], float(c["mean"]), k, float(c["logNoise"]), exact).update_cholesky()
            assert g.info == 0
            assert np.allclose(g.alpha, c["alpha"], rtol=tol * 10, atol=tol), name
            assert abs(g.mll() - float(c["mll"])) <= tol * max(1.0, abs(float(c["mll"]))), name
            mu, var = g.prediction(c["Xt"])
            assert np.allclose(mu, c["mu"], rtol=tol, atol=tol), name
            assert np.allclose(var, c["var"], rtol=tol * 10, atol=tol), name
        assert np.allclose(np.tril(g.factors) @ np.tril(g.factors).T, g.noisy_kernel(), rtol=1e-12, atol=1e-13)


def test_oracle_matches_mpmath_across_a_tile_edge(golden_dir):
    """n = 160 (the blocked factorisation of the HIP path crosses its 128-tile edge there) for the three kernel kinds, test
    rows AT training inputs, 1e-7 away from them and elsewhere: where sigma^2 = k** + noise - |V|^2 cancels three to four
    digits.  50-digit mpmath values (tests/golden/make_golden.py: gp_edge_cases)."""
    z = np.load(os.path.join(golden_dir, "gp_edge.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    assert sorted(int(c["kind"]) for c in cases.values()) == [0, 1, 2]
    for name, c in cases.items():
        assert c["X"].shape[0] == 160 and np.array_equal(c["Xt"][:3], c["X"][[5, 127, 128]])
        g = ogp.GaussianProcess(c["X"], c["y"], float(c["mean"]), ogp.make_kernel(int(c["kind"]), c["loghyp"]), float(c["logNoise"]),
                                True).update_cholesky()
        assert g.info == 0
        assert abs(g.mll() - float(c["mll"])) <= 1e-10 * abs(float(c["mll"])), name
        assert np.max(np.abs(g.alpha - c["alpha"])) <= 1e-7 * np.max(np.abs(c["alpha"])), name
        mu, var = g.prediction(c["Xt"])
        assert np.allclose(mu, c["mu"], rtol=1e-9, atol=1e-11), name
        assert np.allclose(var, c["var"], rtol=1e-8, atol=1e-12), name
        kss = np.diag(ogp.kernelmatrix(g.kernel, c["Xt"][:6], c["Xt"][:6], exact=True))
        assert np.all(c["var"][:6] < 0.05 * kss)          # the rows at / next to training inputs really cancel: var << k**


def test_kernel_forms():
    X = uniform(1, 0, 12).reshape((4, 3), order="F")
    Y = uniform(2, 0, 15).reshape((5, 3), order="F")
    k = ogp.IsoSE(np.log(0.5), np.log(1.5))
    K = ogp.kernelmatrix(k, X, Y, exact=True)
    for i in range(4):
        for j in range(5):
            assert abs(K[i, j] - 2.25 * np.exp(-0.5 * np.sum((X[i] - Y[j]) ** 2) / 0.25)) < 1e-14
    assert np.allclose(ogp.kernelmatrix(k, X, Y), K, rtol=0, atol=1e-14)
    # ArdSE is ADDITIVE over dimensions (src/kernels.jl:39-49): diagonal = sigma^2 * D
    ka = ogp.ArdSE(np.log([0.3, 0.6, 0.9]), np.log(1.2))
    Ka = ogp.kernelmatrix(ka, X, None, exact=True)
    assert np.allclose(np.diag(Ka), 1.44 * 3)
    ref = sum(np.exp(-0.5 * (X[:, d][:, None] - X[:, d][None, :]) ** 2 / [0.09, 0.36, 0.81][d]) for d in range(3)) * 1.44
    assert np.allclose(Ka, ref, rtol=1e-14)
    kl = ogp.IsoLinear(np.log(2.0))
    assert np.allclose(ogp.kernelmatrix(kl, X, Y), X @ Y.T / 4.0)
    assert np.allclose(ogp.prior_diag(kl, X), np.sum(X * X, 1) / 4.0)


def test_chol_continue_equals_potrf():
    rng = np.random.default_rng(0)
    for n, p in ((40, 10), (64, 1), (33, 32), (20, 0), (17, 17)):
        B = rng.standard_normal((n, n))
        A = B @ B.T + n * np.eye(n)
        full = np.linalg.cholesky(A)
        F = A.copy()
        F[:p, :p] = full[:p, :p] if p else F[:p, :p]
        G, info = ogp.chol_continue(F, p + 1)
        assert info == 0
        assert np.max(np.abs(G - full)) < 1e-12 * np.max(np.abs(full))


def test_gradients_match_finite_differences():
    """Reference IsoSE gradients are d mll/d log{l,s} times an extra exp(logs); d/d logNoise is exact;
    ArdSE lengthscale gradients are identically zero."""
    n, D = 30, 2
    X = uniform(5, 0, n * D).reshape((n, D), order="F")
    y = np.sin(4 * X[:, 0]) + 0.1 * normal(6, 0, n)

    def mll_at(kind, h, ln):
        g = ogp.GaussianProcess(X, y, 0.1, ogp.make_kernel(kind, h), ln, True).update_cholesky()
        return g.mll()

    h = np.array([np.log(0.6), 0.3])
    ln = -0.9
    g = ogp.GaussianProcess(X, y, 0.1, ogp.make_kernel(0, h), ln, True).update_cholesky()
    dl, ds, dn = g.grad()
    e = 1e-6
    fd_l = (mll_at(0, h + [e, 0], ln) - mll_at(0, h - [e, 0], ln)) / (2 * e)
    fd_s = (mll_at(0, h + [0, e], ln) - mll_at(0, h - [0, e], ln)) / (2 * e)
    fd_n = (mll_at(0, h, ln + e) - mll_at(0, h, ln - e)) / (2 * e)
    s = np.exp(h[1])
    assert abs(dl - s * fd_l) < 1e-5 * max(1, abs(dl))
    assert abs(ds - s * fd_s) < 1e-5 * max(1, abs(ds))
    assert abs(dn - fd_n) < 1e-5 * max(1, abs(dn))
    ha = np.array([np.log(0.5), np.log(0.8), 0.2])
    ga = ogp.GaussianProcess(X, y, 0.1, ogp.make_kernel(1, ha), ln, True).update_cholesky()
    v = ga.grad()
    assert np.all(np.abs(v[:2]) < 1e-10)
    fd_sa = (mll_at(1, ha + [0, 0, e], ln) - mll_at(1, ha - [0, 0, e], ln)) / (2 * e)
    assert abs(v[2] - np.exp(ha[2]) * fd_sa) < 1e-5 * max(1, abs(v[2]))
    hl = np.array([np.log(0.7), 0.0])
    gl = ogp.GaussianProcess(X, y, 0.1, ogp.make_kernel(2, hl), ln, True).update_cholesky()
    vl = gl.grad()
    fd_ll = (mll_at(2, hl + [e, 0], ln) - mll_at(2, hl - [e, 0], ln)) / (2 * e)
    assert abs(vl[0] - fd_ll) < 1e-5 * max(1, abs(vl[0])) and vl[1] == 0.0


class _N:
    pass


def _leaf(i, obs):
    n = _N()
    n.kind, n.leaf, n.obs, n.children, n.id = "gp", i, np.asarray(obs), [], f"g{i}"
    n.kernelid, n.nobs = 0, len(obs)
    return n


def test_mixture_identity_and_poe_rules():
    """predict of a sum node equals the direct mixture moments; PoE/gPoE/rBCM formulas."""
    n = 25
    X = uniform(11, 0, n).reshape(-1, 1)
    y = np.cos(5 * X[:, 0]) + 2.0
    Xt = uniform(12, 0, 7).reshape(-1, 1)
    k = ogp.IsoSE(np.log(0.4), 0.0)
    halves = [np.arange(0, 15), np.arange(8, 25), np.arange(0, 25)]
    gps = [ogp.GaussianProcess(X[h], y[h], float(np.mean(y[h])), k, -1.0, True).update_cholesky() for h in halves]
    leaves = [_leaf(i, h) for i, h in enumerate(halves)]
    s = _N()
    s.kind, s.children, s.id, s.of_gps = "sum", leaves, "s", False
    w = np.array([0.2, 0.5, 0.3])
    s.logweights = np.log(w)
    mu, var = ospn.predict(s, gps, Xt)
    ms = np.array([g.prediction(Xt)[0] for g in gps])
    vs = np.array([g.prediction(Xt)[1] for g in gps])
    m_direct = (w[:, None] * ms).sum(0)
    v_direct = (w[:, None] * (vs + ms ** 2)).sum(0) - m_direct ** 2
    assert np.allclose(mu, m_direct, rtol=1e-12) and np.allclose(var, v_direct, rtol=1e-10, atol=1e-13)
    p = _N()
    p.kind, p.children, p.id = "split", leaves, "p"
    t = 1.0 / vs
    m_poe, v_poe = ospn.predict_poe(p, gps, Xt)
    assert np.allclose(v_poe, 1.0 / t.sum(0)) and np.allclose(m_poe, (t * ms).sum(0) / t.sum(0))
    m_g, v_g = ospn.predict_gpoe(p, gps, Xt)
    assert np.allclose(v_g, 3.0 / t.sum(0)) and np.allclose(m_g, m_poe)
    m_r, v_r = ospn.predict_rbcm(p, gps, Xt)
    sp = 1.0 + np.exp(-2.0)
    beta = 0.5 * (np.log(sp) - np.log(vs))
    C = 1.0 / sp + (beta * t - beta / sp).sum(0)
    assert np.allclose(v_r, 1.0 / C) and np.allclose(m_r, (beta * t * ms).sum(0) / C)
    # update!: posterior weights proportional to exp(child mll)/K
    z = ospn.update(s, gps)
    ml = np.array([g.mll() for g in gps])
    assert abs(z - (np.log(np.mean(np.exp(ml - ml.max()))) + ml.max())) < 1e-12
    assert abs(np.exp(s.logweights).sum() - 1) < 1e-12


def _advchol(golden_dir):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_advchol", os.path.join(golden_dir, "make_advchol.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    z = np.load(os.path.join(golden_dir, "advchol.npz"))
    return mod, z


def test_chol_continue_on_the_reference_self_check_construction(golden_dir):
    """The reference's own executable checks for this path (src/AdvancedCholeskey.jl:121-135 test_chol_continue,
    :61-110 lrtest) rebuilt with the portable generator: potrf of the leading P x P block + chol_continue!(A, P+1)
    must equal the Cholesky factor of the whole genCov matrix (fixture: LAPACK dpotrf, mpmath-checked at D = 100)."""
    mod, z = _advchol(golden_dir)
    for name in ("cont_d100_p10", "cont_d192_p150"):
        D, P, seed = int(z[f"{name}/D"]), int(z[f"{name}/P"]), int(z[f"{name}/seed"])
        S = mod.gen_cov(D, seed)
        A = S.copy()
        C, info = sla.lapack.dpotrf(A[:P, :P], lower=1, clean=1)     # LAPACK.potrf!('L', view(A.data, 1:P, 1:P))  :129
        assert info == 0
        A[:P, :P] = C
        L, info = ogp.chol_continue(A, P + 1)                        # :130
        assert info == 0
        assert np.max(np.abs(L - z[f"{name}/L"])) <= 1e-13 * np.max(np.abs(z[f"{name}/L"]))
        assert np.sum(np.abs(L - np.linalg.cholesky(S))) < 1e-10     # the quantity test_chol_continue returns (:134)
    # lrtest: the factor the row-deletion update must reproduce is cholesky(B), B = A[idx, idx]
    D, seed = int(z["lr/D"]), int(z["lr/seed"])
    A = mod.gen_cov(D, seed)
    miss = mod.missing_rows(D, seed + 1)
    assert np.array_equal(miss, z["lr/missing"]) and miss.size == 10 and miss.max() < D - 1
    idx = np.setdiff1d(np.arange(D), miss)
    C, info = sla.lapack.dpotrf(A[np.ix_(idx, idx)], lower=1, clean=1)
    assert info == 0 and np.allclose(np.diag(C), z["lr_B/diag"], rtol=1e-13)
    assert abs(2 * np.sum(np.log(np.diag(C))) - float(z["lr_B/logdet"])) < 1e-10


def test_oracle_gradients_match_the_50_digit_references(golden_dir):
    """tests/golden/gp_grad.npz (make_grad_golden.py): gradients contracted directly at 50 digits, in the library's
    convention.  oracle.gp (DenseGP for ArdLinear) within 16 cond_2(K_y) eps max(1, |g|_inf) of every component; the ArdSE
    length-scale slots are the reference's zeros.  Leaf sizes 1, 2, 127..129, 160; D up to 48; the weak-signal cases too."""
    from dense_gp import DenseGP

    z = np.load(os.path.join(golden_dir, "gp_grad.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    assert sorted(set(int(c["kind"]) for c in cases.values())) == [0, 1, 2, 3]
    eps = np.finfo(np.float64).eps
    for name, c in cases.items():
        kind, h, ln = int(c["kind"]), c["loghyp"], float(c["logNoise"])
        if kind == 3:
            g = DenseGP(3, np.append(h, ln), c["X"], c["y"], float(c["mean"]))
        else:
            g = ogp.GaussianProcess(c["X"], c["y"], float(c["mean"]), ogp.make_kernel(kind, h), ln, True).update_cholesky()
        assert g.info == 0
        v = g.grad()
        ref = c["grad"]
        assert v.shape == ref.shape, name
        tol = 16 * float(c["cond"]) * eps * max(1.0, float(np.max(np.abs(ref))))
        assert np.max(np.abs(v - ref)) <= tol, (name, v, ref, tol)
        assert abs(g.mll() - float(c["mll"])) <= 16 * float(c["cond"]) * eps * max(1.0, abs(float(c["mll"]))), name
        if kind == 1:
            assert np.all(ref[:c["X"].shape[1]] == 0.0) and c["grad_true"].shape == (c["X"].shape[1],)


def test_oracle_prediction_aggregation_and_scores_match_the_50_digit_references(golden_dir):
    """tests/golden/gp_pred.npz (make_pred_golden.py): the float64 oracle within 16 cond_2(K_y) eps of the 50-digit moments --
    relative to max(1, max|y|) for mu and to max(1, k** + noise) for sigma^2 -- and its mll as for the gradients.  The
    leaf table's aggregations (the formula of tests/pred_tolerance.py in float64) and the scores (oracle.scores), and config 1
    through oracle/spn.py's update! and literal predict recursion on the tree of oracle/tree.py, within those per-entry bounds
    carried through the formula (pred_tolerance.agg_tol / score_tol)."""
    import math
    import dense_kernels as dk
    from dense_gp import DenseGP
    from oracle import scores as oscores, tree as otree
    from pred_tolerance import agg_tol, aggregate, row_entries, score_tol

    eps = np.finfo(np.float64).eps
    z = np.load(os.path.join(golden_dir, "gp_pred.npz"))
    single, T, C = {}, {}, {}
    for key in z.files:
        head, rest = key.split("/", 1)
        if head == "single":
            name, field = rest.split("/")
            single.setdefault(name, {})[field] = z[key]
        else:
            (T if head == "table" else C)[rest] = z[key]

    def leaf(kind, hyp, X, y, mean):
        if kind == 3:
            return DenseGP(3, hyp, X, y, mean)
        return ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, hyp[:-1]), hyp[-1], True).update_cholesky()

    def moments_tol(cond, kss, noise, yscale):
        b = 16 * np.asarray(cond) * eps
        return b * yscale, b * np.maximum(1.0, np.asarray(kss) + noise)

    assert sorted(set(int(c["kind"]) for c in single.values())) == [0, 1, 2, 3]
    for name, c in single.items():
        kind = int(c["kind"])
        hyp = np.concatenate([c["loghyp"], [float(c["logNoise"])]])
        g = leaf(kind, hyp, c["X"], c["y"], float(c["mean"]))
        assert g.info == 0
        mu, var = g.prediction(c["Xt"])
        tm, tv = moments_tol(float(c["cond"]), c["kss"], np.exp(2 * hyp[-1]), max(1.0, float(np.max(np.abs(c["y"])))))
        assert np.all(np.abs(mu - c["mu"]) <= tm) and np.all(np.abs(var - c["var"]) <= tv), name
        assert abs(g.mll() - float(c["mll"])) <= 16 * float(c["cond"]) * eps * max(1.0, abs(float(c["mll"]))), name
    # the leaf table: per entry, both target variants
    L = T["kid"].size
    rp, op_ = T["route_ptr"], T["obs_ptr"]
    nt = T["Xt"].shape[0]
    mu_o, mu_off_o, var_o = np.zeros(rp[-1]), np.zeros(rp[-1]), np.zeros(rp[-1])
    tmu, tmu_off, tvar = np.zeros(rp[-1]), np.zeros(rp[-1]), np.zeros(rp[-1])
    for l in range(L):
        k = int(T["kid"][l])
        kind, hyp = int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]]
        o = T["obs_idx"][op_[l]:op_[l + 1]]
        rows = T["route_idx"][rp[l]:rp[l + 1]]
        sl = slice(rp[l], rp[l + 1])
        for off, mean, mll, mref, mo, tmo in ((0.0, T["mean"], T["mll"], T["mu"], mu_o, tmu),
                                              (1000.0, T["mean_off"], T["mll_off"], T["mu_off"], mu_off_o, tmu_off)):
            y = T["y"] + off
            g = leaf(kind, hyp, T["X"][o], y[o], float(mean[l]))
            assert g.info == 0 and abs(g.mll() - mll[l]) <= 16 * T["cond"][l] * eps * max(1.0, abs(mll[l])), l
            if rows.size:
                mo[sl], var_o[sl] = g.prediction(T["Xt"][rows])
                tmo[sl], tvar[sl] = moments_tol(T["cond"][l], T["kss"][sl], np.exp(2 * hyp[-1]), max(1.0, float(np.max(np.abs(y)))))
                assert np.all(np.abs(mo[sl] - mref[sl]) <= tmo[sl]) and np.all(np.abs(var_o[sl] - T["var"][sl]) <= tvar[sl]), l
    # aggregations in float64 from the oracle's moments, and the oracle's scores of them
    ent = row_entries(rp, T["route_idx"], nt)
    pk = int(T["prior_kid"])
    kss_prior = dk.prior_diag(3, T["hyp"][pk][:T["hyp_len"][pk] - 1], T["Xt"])
    noise_prior = float(np.exp(2.0 * T["hyp"][pk][T["hyp_len"][pk] - 1]))
    fams = dict(mixture=(0, T["w_mix"], False), mixture_plain=(0, T["w_mix"], True), poe=(1, np.ones(L), False),
                gpoe=(2, T["beta"], False), rbcm=(3, None, False), mixture_off=(0, T["w_mix"], False))
    for fam_name, (fam, coef, plain) in fams.items():
        off = fam_name == "mixture_off"
        m_in, tm_in = (mu_off_o, tmu_off) if off else (mu_o, tmu)
        kw = dict(coef=coef, group=T["group"], G=int(T["G"]), plain=plain, noise_prior=noise_prior)
        am, av = aggregate(fam, list(m_in), list(var_o), ent, kss_prior=list(kss_prior), log=math.log, **kw)
        am, av = np.array(am, dtype=np.float64), np.array(av, dtype=np.float64)
        tm, tv = agg_tol(fam, m_in, var_o, tm_in, tvar, ent, S1=T.get(f"agg/{fam_name}/S1"), kss_prior=kss_prior, **kw)
        assert np.all(np.abs(am - T[f"agg/{fam_name}/mu"]) <= tm) and np.all(np.abs(av - T[f"agg/{fam_name}/var"]) <= tv), fam_name
        yt = T["yt"] + (1000.0 if off else 0.0)
        sc = [oscores.mse(yt, am), oscores.sse(yt, am), oscores.mae(yt, am), oscores.sae(yt, am), oscores.nlpd(yt, am, av)]
        ts = score_tol(yt, T[f"agg/{fam_name}/mu"], T[f"agg/{fam_name}/var"], tm, tv)
        assert np.all(np.abs(np.array(sc) - T[f"agg/{fam_name}/scores"]) <= ts), fam_name
    # config 1: the reference's tree builder, update! and literal predict recursion, all in the oracle
    x, y, xt = C["x"], C["y"], C["xt"]
    X = x.reshape(-1, 1)
    root = otree.spn_nodes(otree.build_tree(X, y, 10, 4, 3, 2, 0.5, True, meanFun=float(np.mean(x)), seed=11), 0, [1.0, 1.0], 1.0)
    gps = ospn.make_leaf_gps(root, X, y, exact_dist=True)
    for g in gps:
        g.update_cholesky()
    lm = np.array([g.mll() for g in gps])
    ltol = 16 * C["cond"] * eps * np.maximum(1.0, np.abs(C["leaf_mll"]))
    assert np.all(np.abs(lm - C["leaf_mll"]) <= ltol)
    zr = ospn.update(root, gps)
    assert abs(zr - float(C["root_mll"])) <= np.sum(ltol) + 16 * eps * abs(float(C["root_mll"]))
    mu, var = ospn.predict(root, gps, xt)
    noise = np.exp(2.0)
    tm_e, tv_e = moments_tol(np.repeat(C["cond"], np.diff(C["route_ptr"])), np.full(C["leaf_var"].size, noise), noise,
                             max(1.0, float(np.max(np.abs(y)))))
    ent = row_entries(C["route_ptr"], C["route_idx"], xt.shape[0])
    tm, tv = agg_tol(0, C["leaf_mu"], C["leaf_var"], tm_e, tv_e, ent, S1=C["S1"], coef=C["leaf_w"])
    assert np.all(np.abs(mu - C["mu"]) <= tm) and np.all(np.abs(var - C["var"]) <= tv)
    sc = [oscores.mse(C["yt"], mu), oscores.sse(C["yt"], mu), oscores.mae(C["yt"], mu), oscores.sae(C["yt"], mu),
          oscores.nlpd(C["yt"], mu, var)]
    assert np.all(np.abs(np.array(sc) - C["scores"]) <= score_tol(C["yt"], C["mu"], C["var"], tm, tv))
