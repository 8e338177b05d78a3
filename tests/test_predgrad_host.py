"""CPU tests of the predict-gradient path: what tests/golden/gp_predgrad.npz covers, the dense float64 helper
(tests/predgrad_dense.py) against its 50 digits and against central differences of its own mu and sigma^2, the host aggregation
`aggregate_input_gradients` against the 50-digit aggregate cases and against central differences of the aggregation formula
(pred_tolerance.aggregate) for every family, its exact rules, and the refusals.  No device."""
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import datagen, hipabi
import dense_kernels as dk
import predgrad_dense as pgd
from pred_tolerance import EPS, Prop, aggregate, moment_tol, row_entries

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TABLE = {k.split("/", 1)[1]: v for k, v in np.load(os.path.join(GOLDEN, "gp_pred.npz")).items() if k.startswith("table/")}


Z = np.load(os.path.join(GOLDEN, "gp_predgrad.npz"))
CASE_NAMES = sorted(k[:-5] for k in Z.files if k.endswith("/meta"))
AGG = {"mixture": (0, False), "plain": (0, True), "poe": (1, False), "gpoe": (2, False), "rbcm": (3, False)}


def test_fixture_covers_the_cases_the_feature_names():
    cases = {n: pgd.case_inputs(Z, n) for n in CASE_NAMES}
    shapes = {(c["X"].shape[0], c["Xt"].shape[0]) for c in cases.values()}
    assert {(1, 1), (5, 3), (127, 128), (130, 129), (300, 260)} <= shapes
    for kind in range(9):
        mine = [c for c in cases.values() if c["kind"] == kind]
        for D in (1, 3):
            assert {(1, 1), (5, 3), (127, 128), (130, 129), (300, 260)} <= {(c["X"].shape[0], c["Xt"].shape[0]) for c in mine
                                                                             if c["X"].shape[1] == D}
        assert any(c["X"].shape[1] == 40 for c in mine) == (kind in (0, 4))
    assert max(float(np.max(np.abs(c["y"]))) for c in cases.values()) > 500.0
    for name, c in cases.items():
        nt = c["Xt"].shape[0]
        assert c["mean"] != 0.0 and abs(c["mean"] - float(np.mean(c["y"]))) > 0.1
        assert c["cond"] <= 1e6
        assert any(np.array_equal(c["Xt"][0], x) for x in c["X"])                      # Delta = 0
        a, b = c["dup"]
        assert np.array_equal(c["Xt"][a], c["Xt"][b]) and (a != b or nt == 1) and a // 128 == b // 128
        assert np.array_equal(c["dmu"][a], c["dmu"][b]) and np.array_equal(c["dvar"][a], c["dvar"][b])
        if c["kind"] not in dk.LINEAR and nt > 4:                                      # k* underflows: exactly 0
            assert c["far"] == [2, 3] and np.all(c["Xt"][2] == 1e3) and np.all(c["Xt"][3] == -1e3)
            assert np.all(c["dmu"][2:4] == 0.0) and np.all(c["dvar"][2:4] == 0.0)
        else:
            assert c["far"] == []
    for f in AGG:
        assert Z["agg/" + f].shape == (120, 6)
    assert os.path.getsize(os.path.join(GOLDEN, "gp_predgrad.npz")) <= os.path.getsize(os.path.join(GOLDEN, "gp_pred.npz"))


@pytest.mark.parametrize("kind", range(9))
def test_dense_helper_against_50_digits(kind):
    """The float64 helper with its own Cholesky, within the tolerance of the 50 digits on every case of the kind (the worst
    ratio over all cases is recorded in DESIGN.md); the far rows come out exactly 0."""
    worst = 0.0
    for name in [n for n in CASE_NAMES if n.startswith(KIND_NAMES[kind] + "_")]:
        c = pgd.case_inputs(Z, name)
        _, _, dmu, dvar = pgd.moments(kind, c["loghyp"], c["logNoise"], c["X"], c["y"], c["mean"], c["Xt"])
        tm, tv = pgd.tolerances(kind, c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], c["dmu"], c["dvar"])
        r = max(float(np.max(np.abs(dmu - c["dmu"]) / tm)), float(np.max(np.abs(dvar - c["dvar"]) / tv)))
        print(f"\n{name}: cond {c['cond']:.3g}, dense err/tol {r:.3g}")
        worst = max(worst, r)
        assert r <= 1.0, (name, r)
        for p in c["far"]:
            assert np.all(dmu[p] == 0.0) and np.all(dvar[p] == 0.0)
    print(f"kind {kind}: worst dense err/tol {worst:.3g}")


KIND_NAMES = ["isose", "ardse", "isolinear", "ardlinear", "ardseproduct", "isomatern32", "isomatern52", "ardmatern32", "ardmatern52"]


def _agg_case(fname):
    """The inputs of an aggregate case: the table's own per-entry mu, var at the stored entries, the stored per-entry gradients,
    the rows' (leaf, entry) lists, and the family's arguments."""
    T = TABLE
    fam, plain = AGG[fname]
    sel = Z["agg/entries"].astype(np.int64)
    rp, ri = T["route_ptr"], T["route_idx"]
    R, D = Z["agg/" + fname].shape[0], T["X"].shape[1]
    leaf = np.searchsorted(rp, sel, side="right") - 1
    ent = [[] for _ in range(R)]
    for k, e in enumerate(sel):
        ent[int(ri[e])].append((int(leaf[k]), k))
    kw = dict(plain=plain)
    pk = int(T["prior_kid"])
    phyp = T["hyp"][pk][:T["hyp_len"][pk]]
    if fam == 0:
        kw["coef"] = T["w_mix"]
    elif fam == 1:
        kw["coef"] = np.ones(T["kid"].size)
    elif fam == 2:
        kw["coef"] = T["beta"]
    else:
        Xt = T["Xt"][:R]
        kw.update(group=T["group"], G=int(T["G"]), kss_prior=dk.prior_diag(int(T["kinds"][pk]), phyp[:-1], Xt),
                  noise_prior=float(np.exp(2 * phyp[-1])), dkss_prior=dk.prior_dx(int(T["kinds"][pk]), phyp[:-1], Xt))
    d = Z["agg/dleaf"]
    return fam, T["mu"][sel], T["var"][sel], d[:, :D], d[:, D:], ent, kw, sel, leaf


@pytest.mark.parametrize("fname", sorted(AGG))
def test_aggregation_against_50_digits(fname):
    """aggregate_input_gradients on the stored float64 inputs against the 50-digit aggregate of exactly those inputs.  The
    inputs are exact here, so the tolerance is the function's own rounding: every input carries 4 eps of its magnitude through
    the formula (Prop, as agg_tol carries the per-entry tolerances), plus 64 eps of the result."""
    fam, mu, var, dmu, dvar, ent, kw, _, _ = _agg_case(fname)
    ref = Z["agg/" + fname]
    D = dmu.shape[1]
    gm, gv = dsm.aggregate_input_gradients(fam, mu, var, dmu, dvar, ent, **kw)
    P = lambda a: [Prop(v, 4 * EPS * abs(v)) for v in a]                                # noqa: E731
    pkw = dict(kw)
    if fam == 3:
        pkw.update(kss_prior=P(kw["kss_prior"]), dkss_prior=[P(r) for r in kw["dkss_prior"]])
    tm, tv = pgd.aggregate_gradients(fam, P(mu), P(var), [P(r) for r in dmu], [P(r) for r in dvar], ent, log=Prop.log, **pkw)
    tol_m = np.array([[float(Prop.of(v).e) for v in r] for r in tm]) + 64 * EPS * np.abs(ref[:, :D])
    tol_v = np.array([[float(Prop.of(v).e) for v in r] for r in tv]) + 64 * EPS * np.abs(ref[:, D:])
    rm, rv = np.abs(gm - ref[:, :D]) / tol_m, np.abs(gv - ref[:, D:]) / tol_v
    print(f"\n{fname}: worst err/tol dmu {np.max(rm):.3g} dvar {np.max(rv):.3g}; largest tolerance relative to the value "
          f"{np.max(tol_v / np.maximum(np.abs(ref[:, D:]), 1e-300)):.3g}")
    assert np.all(rm <= 1.0) and np.all(rv <= 1.0), (fname, np.max(rm), np.max(rv))


def _case(kind, n, nt, D, seed):
    X = datagen.uniform(seed, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * datagen.normal(seed + 1, 0, n) + 0.7
    Xt = datagen.uniform(seed + 2, 0, nt * D).reshape((nt, D), order="F") * 1.2 - 0.1
    Xt[0] = X[n - 1]                    # Delta = 0
    ls = np.array([0.35, 0.5, 0.42])[:D] * np.sqrt(D) + (0.5 if kind in (2, 3) else 0.0)
    nl = D if kind in dk.ARD else 1
    loghyp = np.concatenate([np.log(ls[:nl]), [0.0 if kind in (2, 3) else 0.1]])
    return X, y, Xt, loghyp, float(np.log(0.1)), float(np.mean(y)) + 0.25


@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("kind", range(9))
def test_dense_helper_against_central_differences(kind, D):
    """Step h = 1e-5 l_d.  A central difference of f carries h^2 |f'''| / 6 of truncation and eps |f| / h of rounding: with
    derivatives of order |f| / l^k that is (1e-10 / 6 + 2.2e-16 / 1e-5) |f| / l_d ~ 4e-11 |f| / l_d per evaluation; the moments
    are sums over n = 40 rows with cancellation (k_t . alpha with |alpha| up to 1 / noise = 100 times the moment's size), so
    the bound is 1e-6 (|f'| + scale / l_d), scale = max(1, max|y|) for mu and max(1, k** + noise) for sigma^2 -- four orders
    above the estimate, five below a wrong formula (an error in a derivative is of order |f'| itself).  Matern 3/2 at
    Delta = 0 has a discontinuous third derivative, so the row AT a training input gets the first-order bound h |f''| instead:
    1e-4 of the same scale."""
    X, y, Xt, loghyp, logNoise, mean = _case(kind, 40, 7, D, seed=7000 + 10 * kind + D)
    mu, var, dmu, dvar = pgd.moments(kind, loghyp, logNoise, X, y, mean, Xt)
    il2 = dk.unpack(kind, loghyp, D)[0]
    yscale = max(1.0, float(np.max(np.abs(y))))
    vscale = np.maximum(1.0, dk.prior_diag(kind, loghyp, Xt) + np.exp(2 * logNoise))
    worst = 0.0
    for d in range(D):
        ld = 1.0 / np.sqrt(il2[d])
        h = 1e-5 * ld
        E = np.zeros_like(Xt)
        E[:, d] = h
        mp_, vp, _, _ = pgd.moments(kind, loghyp, logNoise, X, y, mean, Xt + E)
        mm, vm, _, _ = pgd.moments(kind, loghyp, logNoise, X, y, mean, Xt - E)
        fm, fv = (mp_ - mm) / (2 * h), (vp - vm) / (2 * h)
        rel = np.full(Xt.shape[0], 1e-6)
        if kind in (5, 7):
            rel[0] = 1e-4
        bm = rel * (np.abs(dmu[:, d]) + yscale / ld)
        bv = rel * (np.abs(dvar[:, d]) + vscale / ld)
        worst = max(worst, float(np.max(np.abs(fm - dmu[:, d]) / bm)), float(np.max(np.abs(fv - dvar[:, d]) / bv)))
        assert np.all(np.abs(fm - dmu[:, d]) <= bm), (kind, d, np.max(np.abs(fm - dmu[:, d]) / bm))
        assert np.all(np.abs(fv - dvar[:, d]) <= bv), (kind, d, np.max(np.abs(fv - dvar[:, d]) / bv))
    print(f"\nkind {kind} D {D}: worst central-difference err / bound {worst:.3g}")


def test_far_rows_and_the_row_at_a_training_input():
    """Rows at +-1e3: k* underflows, both gradients are exactly 0 for the stationary kinds; the row AT a training input is finite."""
    for kind in (0, 1, 4, 5, 6, 7, 8):
        X, y, Xt, loghyp, logNoise, mean = _case(kind, 30, 6, 3, seed=7200 + kind)
        Xt[2], Xt[3] = 1e3, -1e3
        _, _, dmu, dvar = pgd.moments(kind, loghyp, logNoise, X, y, mean, Xt)
        assert np.all(dmu[2:4] == 0.0) and np.all(dvar[2:4] == 0.0)
        assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))


def _table_entries(seed, D=2):
    """Per-entry moments and gradients on the routes of the 41-leaf table of gp_pred.npz (values from the counter stream: the
    aggregation is a formula over them, whatever GP they came from)."""
    T = TABLE
    rp, ri = T["route_ptr"], T["route_idx"]
    E, n_t = int(rp[-1]), T["Xt"].shape[0]
    mu = datagen.normal(seed, 0, E)
    var = 0.05 + datagen.uniform(seed + 1, 0, E)
    dmu = datagen.normal(seed + 2, 0, E * D).reshape(E, D)
    dvar = 0.3 * datagen.normal(seed + 3, 0, E * D).reshape(E, D)
    return mu, var, dmu, dvar, row_entries(rp, ri, n_t), n_t


def _family_args(family, L, n_t, D, seed):
    if family == 0:
        w = 0.2 + datagen.uniform(seed, 0, L)
        return dict(coef=w / 7.0), {}
    if family in (1, 2):
        return dict(coef=np.full(L, 1.0 if family == 1 else 0.25)), {}
    group = (np.arange(L) % 3).astype(np.int32)
    kss = 1.5 + datagen.uniform(seed, 0, n_t)
    dk = 0.4 * datagen.normal(seed + 1, 0, n_t * D).reshape(n_t, D)
    return dict(group=group, G=4), dict(kss_prior=kss, noise_prior=0.01, dkss_prior=dk)       # group 3 never sees a row


@pytest.mark.parametrize("family,plain", [(0, False), (0, True), (1, False), (2, False), (3, False)])
def test_aggregation_against_differences_of_the_formula(family, plain):
    """aggregate_input_gradients against central differences of pred_tolerance.aggregate along the direction the per-entry
    gradients define: moving the test point by t e_d moves every entry's moments by t dmu[e, d], t dvar[e, d] (and the prior
    term by t dkss[r, d]).  The formula is smooth in its inputs with derivatives of order 1 here; h = 1e-6 gives a truncation of
    order 1e-12 and a rounding of order 1e-10: the bound is 1e-7 (1 + |value|)."""
    D = 2
    mu, var, dmu, dvar, ent, n_t = _table_entries(7300 + family, D)
    L = TABLE["kid"].size
    args, prior = _family_args(family, L, n_t, D, 7350 + family)
    keep = (mu.copy(), var.copy(), dmu.copy(), dvar.copy())
    gm, gv = dsm.aggregate_input_gradients(family, mu, var, dmu, dvar, ent, plain=plain, **args, **prior)
    for a, b in zip(keep, (mu, var, dmu, dvar)):
        assert np.array_equal(a, b)                                         # inputs are left untouched
    assert gm.shape == (n_t, D) and gv.shape == (n_t, D)
    h = 1e-6
    seen_rows = np.array([len(er) > 0 for er in ent])

    def f(t, d):
        kw = dict(args)
        if family == 3:
            kw.update(kss_prior=list(prior["kss_prior"] + t * prior["dkss_prior"][:, d]), noise_prior=prior["noise_prior"])
        m, v = aggregate(family, list(mu + t * dmu[:, d]), list(var + t * dvar[:, d]), [er for er in ent if er], plain=plain,
                         log=np.log, **kw) if family != 3 else _agg_rbcm(kw, mu + t * dmu[:, d], var + t * dvar[:, d], ent)
        return np.array(m, dtype=np.float64), np.array(v, dtype=np.float64)

    for d in range(D):
        (mp_, vp), (mm, vm) = f(h, d), f(-h, d)
        fm, fv = (mp_ - mm) / (2 * h), (vp - vm) / (2 * h)
        assert np.all(np.abs(fm - gm[seen_rows, d]) <= 1e-7 * (1 + np.abs(fm))), np.max(np.abs(fm - gm[seen_rows, d]))
        assert np.all(np.abs(fv - gv[seen_rows, d]) <= 1e-7 * (1 + np.abs(fv))), np.max(np.abs(fv - gv[seen_rows, d]))


def _agg_rbcm(kw, mu, var, ent):
    rows = [r for r, er in enumerate(ent) if er]
    return aggregate(3, list(mu), list(var), [ent[r] for r in rows], group=kw["group"], G=kw["G"],
                     kss_prior=[kw["kss_prior"][r] for r in rows], noise_prior=kw["noise_prior"], log=np.log)


def test_clamped_leaf_variance_is_a_constant():
    """sigma2_l <= 0 -> 1e-8 in the mixture: that leaf contributes dsigma2_l = 0 (its mean term stays)."""
    ent = [[(0, 0), (1, 1)]]
    mu, var = np.array([0.3, -0.2]), np.array([-1e-12, 0.5])
    dmu, dvar = np.array([[1.0, 2.0], [0.5, -1.0]]), np.array([[7.0, 7.0], [0.25, 0.5]])
    w = np.array([0.4, 0.6])
    gm, gv = dsm.aggregate_input_gradients(0, mu, var, dmu, dvar, ent, coef=w)
    m = w @ mu
    assert np.allclose(gm[0], w @ dmu, rtol=0, atol=1e-15)
    ref = w[1] * dvar[1] + 2.0 * (w[0] * (mu[0] - m) * dmu[0] + w[1] * (mu[1] - m) * dmu[1])
    assert np.allclose(gv[0], ref, rtol=0, atol=1e-15)


def test_rbcm_skips_groups_that_did_not_see_the_row():
    """The result does not depend on how many empty groups the model has."""
    mu, var, dmu, dvar, ent, n_t = _table_entries(7400)
    L = TABLE["kid"].size
    group = (np.arange(L) % 3).astype(np.int32)
    kss, dk = np.full(n_t, 1.2), np.zeros((n_t, 2))
    a = dsm.aggregate_input_gradients(3, mu, var, dmu, dvar, ent, group=group, G=3, kss_prior=kss, noise_prior=0.01, dkss_prior=dk)
    b = dsm.aggregate_input_gradients(3, mu, var, dmu, dvar, ent, group=group, G=6, kss_prior=kss, noise_prior=0.01, dkss_prior=dk)
    rows = np.array([len(er) > 0 for er in ent])
    assert np.array_equal(a[0][rows], b[0][rows]) and np.array_equal(a[1][rows], b[1][rows])
    assert np.all(np.isfinite(a[0][rows])) and np.all(np.isfinite(a[1][rows]))


def test_refusals():
    from oracle_context import OracleContext
    X, y, Xt = dsm.regression_data(300, 2, n_test=5, seed=11)
    model = dsm.buildDSMGP(X, y, 2, 2, M=60, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.1), seed=3, ctx=OracleContext())
    node = model.root
    while node.kind != "sum":
        node = node.children[0]
    node.logweights = node.logweights + 0.3               # weights that no longer add up to one
    with pytest.raises(ValueError, match="not normalised"):
        dsm.predict_gradients(model, Xt)
    model2 = dsm.buildDSMGP(X, y, 2, 2, M=60, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.1), seed=3, ctx=OracleContext())
    with pytest.raises(NotImplementedError, match="has no predict_gradients"):         # a context without the device call
        dsm.predict_gradients(model2, Xt)
    world = model2.shard.world
    model2.shard.world = 2
    try:
        with pytest.raises(NotImplementedError, match="several ranks"):
            dsm.predict_gradients(model2, Xt)
    finally:
        model2.shard.world = world
    sc = hipabi.StreamingContext.__new__(hipabi.StreamingContext)
    with pytest.raises(hipabi.DsmgpError) as e:
        sc.predict_gradients()
    assert e.value.code == hipabi.E_STATE
