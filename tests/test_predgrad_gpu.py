"""GPU tests of dsmgp_predict_gradients: the gradients of the predictive mean and variance of every (leaf, routed row)
entry with respect to the test point (tile_predbeta_kernel, pred_inputgrad_kernel, pred_inputgrad_finish_kernel).

Reference of the single-leaf cases: tests/golden/gp_predgrad.npz (50 digits, tests/golden/make_predgrad_golden.py), within
predgrad_dense.tolerances (RTOL relative + ATOL times the quantity's scale times g_d).  The leaf table and the larger single GP
are compared with the dense float64 helper tests/predgrad_dense.py fed with download_factor of the same context, within twice
that tolerance because both sides carry float64 rounding."""
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import datagen
import dense_kernels as dk
import predgrad_dense as pgd
from test_predcov_gpu import TABLE, _same_bits, _table_setup, lib_noise

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_predgrad.npz"))
CASE_NAMES = sorted(k[:-5] for k in Z.files if k.endswith("/meta"))

SHAPES = [(1, 1), (5, 3), (127, 128), (130, 129), (300, 260)]
KIND_NAMES = ["isose", "ardse", "isolinear", "ardlinear", "ardseproduct", "isomatern32", "isomatern52", "ardmatern32", "ardmatern52"]
FAR = 1e3


def loghyp_of(kind, D):
    """The library's hyper-vector without the noise; length-scales grow with sqrt(D) so that cond(K_y) stays below 1e6."""
    ls = np.array([0.35, 0.5, 0.42])[:D] * np.sqrt(D) if D <= 3 else np.full(D, 0.3 * np.sqrt(D))
    if kind in (2, 3):
        ls = ls + 0.5
    nl = D if kind in dk.ARD else 1
    return np.concatenate([np.log(ls[:nl]), [0.0 if kind in (2, 3) else 0.1]])


def make_case(kind, n, nt, D, seed, yscale=1.0):
    X = datagen.uniform(seed, 0, n * D).reshape((n, D), order="F")
    y = yscale * (np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * datagen.normal(seed + 1, 0, n)) + 0.7 * yscale
    Xt = datagen.uniform(seed + 2, 0, nt * D).reshape((nt, D), order="F") * 1.2 - 0.1
    Xt[0] = X[n - 1]                                # a test row AT a training row
    far = []
    if nt > 4:
        if kind not in (2, 3):
            Xt[2], Xt[3] = FAR, -FAR
            far = [2, 3]
        Xt[4] = Xt[1]                               # one row listed twice, in ONE 128-row tile: the sweep that forms K_tn L^-T may
                                                    # split the sums of different row tiles differently (its last bits differ there)
    dup = (1, 4) if nt > 4 else ((0, nt - 1) if nt > 1 else (0, 0))
    if 4 >= nt > 1:
        Xt[nt - 1] = Xt[0]
    return dict(kind=kind, X=np.asfortranarray(X), y=y, Xt=np.asfortranarray(Xt), mean=float(np.mean(y)) + 0.25,
                loghyp=loghyp_of(kind, D), logNoise=float(np.log(0.1)), far=far, dup=dup)


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _single(ctx, c, path):
    X, y, Xt = c["X"], c["y"], c["Xt"]
    n, nt = X.shape[0], Xt.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
    ctx.set_hyper(0, c["kind"], np.concatenate([c["loghyp"], [c["logNoise"]]]))
    if path == "joint":
        ctx.set_test(Xt, [0, nt], np.arange(nt))
        _, info, _ = ctx.fit()
        ctx.predict_run()
    else:
        _, info, _ = ctx.fit()
        ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
    assert info[0] == 0


def _reference(ctx, leaf, c):
    n = c["X"].shape[0]
    F, alpha = ctx.download_factor(leaf, n)
    return pgd.moments(c["kind"], c["loghyp"], c["logNoise"], c["X"], c["y"], c["mean"], c["Xt"], L=np.tril(F), alpha=alpha)


def _check(tag, got, ref, tol):
    err = np.abs(got - ref)
    ratio = err / tol
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert np.all(err <= tol), (tag, w, got[w], ref[w], tol[w])


def _check_case(ctx, c, path, tag):
    _single(ctx, c, path)
    nt, D = c["Xt"].shape
    dmu, dvar = ctx.predict_gradients()
    assert dmu.shape == (nt, D) and dvar.shape == (nt, D) and dmu.flags.f_contiguous and dvar.flags.f_contiguous
    tmu, tvar = pgd.tolerances(c["kind"], c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], c["dmu"], c["dvar"])
    _check(tag + " dmu", dmu, c["dmu"], tmu)
    _check(tag + " dvar", dvar, c["dvar"], tvar)
    # exact properties, on bits
    a, b = c["dup"]
    assert _same_bits(dmu[a], dmu[b]) and _same_bits(dvar[a], dvar[b])
    dmu2, dvar2 = ctx.predict_gradients()
    assert _same_bits(dmu, dmu2) and _same_bits(dvar, dvar2)
    dmu3, none = ctx.predict_gradients(want_var=False)
    assert none is None and _same_bits(dmu, dmu3)
    for p in c["far"]:
        assert np.all(dmu[p] == 0.0) and np.all(dvar[p] == 0.0), (tag, p, dmu[p], dvar[p])


@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("kind", range(9))
def test_fixture_cases_against_50_digits(ctx, kind, path):
    """Every fixture case of the kind (five shapes, D = 1 and 3; D = 40 for IsoSE and ArdSEProduct, whose 40 length-scales are
    EQUAL, so those two cases cannot tell one dimension's factor from another's) on both routes to K_tn L^-T, against the 50
    digits within the tolerance; then the exact properties on bits.  Every kind past one chunk of 8 dimensions with distinct
    length-scales: tests/test_wide_inputs_gpu.py."""
    names = [n for n in CASE_NAMES if n.startswith(KIND_NAMES[kind] + "_")]
    assert len(names) >= 10
    for name in names:
        c = pgd.case_inputs(Z, name)
        assert c["kind"] == kind
        _check_case(ctx, c, path, f"{name} {path}")


def test_other_results_keep_their_bits(ctx):
    """predict_fetch, predict_cov, gradients and loo return the same bits before and after the call."""
    c = make_case(6, 130, 129, 3, seed=6200)
    _single(ctx, c, "standalone")
    nt = c["Xt"].shape[0]
    before = (ctx.predict_fetch(), ctx.predict_cov(0, nt), ctx.gradients(5), ctx.loo())
    _single(ctx, c, "standalone")
    ctx.predict_gradients()
    after = (ctx.predict_fetch(), ctx.predict_cov(0, nt), ctx.gradients(5), ctx.loo())
    for x, y in zip(before, after):
        for p, q in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
            assert _same_bits(p, q)
    d1 = ctx.predict_gradients()            # L^-T is now the arena loo left: read as it is
    _single(ctx, c, "standalone")
    d2 = ctx.predict_gradients()            # ... and filled by the call itself
    assert _same_bits(d1[0], d2[0]) and _same_bits(d1[1], d2[1])


def test_gradient_mask_is_left_alone(ctx):
    """Under a mask of set_gradient_leaves that leaves a factor owner out, the call inverts every owner over lists of its own:
    dsmgp_gradients returns the same bits with and without the call in between, and the call's results do not depend on the mask."""
    T = TABLE
    rp, ri = T["route_ptr"], T["route_idx"]
    L = T["kid"].size
    mask = np.zeros(L, dtype=np.int32)
    mask[[3, 7]] = 1

    def run(with_call, masked=True):
        _table_setup(ctx)
        ctx.set_gradient_leaves(mask if masked else None)
        ctx.fit()
        ctx.predict_leaves(T["Xt"], rp, ri)
        g0 = ctx.gradients(7)
        d = ctx.predict_gradients() if with_call else None
        return g0, ctx.gradients(7), d

    try:
        a0, a1, _ = run(False)
        b0, b1, d = run(True)
        assert _same_bits(a0, b0) and _same_bits(a1, b1) and _same_bits(a0, a1)
        _, _, d_all = run(True, masked=False)
        assert _same_bits(d[0], d_all[0]) and _same_bits(d[1], d_all[1])
    finally:
        ctx.set_gradient_leaves(None)


def test_multicontext_puts_the_entries_back_in_order(ctx):
    """MultiContext.predict_gradients: the leaves are independent, so every entry is the single context's."""
    T = TABLE
    rp, ri = T["route_ptr"], T["route_idx"]
    ctx.set_option(hipabi.OPT_LANES, 1)
    mc = hipabi.MultiContext(0, n=2)
    try:
        mc.set_option(hipabi.OPT_LANES, 1)
        for c in (ctx, mc):
            _table_setup(c)
            c.fit()
            c.set_test(T["Xt"], rp, ri)
            c.predict_run()
        a, b = ctx.predict_gradients(), mc.predict_gradients()
        _, _, tmu, tvar = _table_reference(ctx)
        # each side is within the per-entry tolerance of the truth (a context with other leaves cuts its sums differently)
        assert np.all(np.abs(a[0] - b[0]) <= 2.0 * tmu) and np.all(np.abs(a[1] - b[1]) <= 2.0 * tvar)
        assert np.any(a[0] != 0.0)
        assert mc.predict_gradients(want_var=False)[1] is None
    finally:
        mc.close()
        ctx.set_option(hipabi.OPT_LANES, 0)


def _table_reference(ctx):
    """(dmu, dvar, tol dmu, tol dvar) over the entries of the 41-leaf table: the dense helper fed with download_factor of `ctx`."""
    T = TABLE
    rp, ri, op_, ob = T["route_ptr"], T["route_idx"], T["obs_ptr"], T["obs_idx"]
    E, D = int(rp[-1]), T["X"].shape[1]
    out = [np.zeros((E, D)) for _ in range(4)]
    for l in range(T["kid"].size):
        if rp[l + 1] == rp[l]:
            continue
        kid = int(T["kid"][l])
        hyp = T["hyp"][kid][:T["hyp_len"][kid]]
        c = dict(kind=int(T["kinds"][kid]), loghyp=hyp[:-1], logNoise=float(hyp[-1]), mean=float(T["mean"][l]),
                 X=np.asfortranarray(T["X"][ob[op_[l]:op_[l + 1]]]), y=T["y"][ob[op_[l]:op_[l + 1]]],
                 Xt=np.asfortranarray(T["Xt"][ri[rp[l]:rp[l + 1]]]))
        _, _, rmu, rvar = _reference(ctx, l, c)
        tmu, tvar = pgd.tolerances(c["kind"], c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], rmu, rvar)
        for o, v in zip(out, (rmu, rvar, tmu, tvar)):
            o[int(rp[l]):int(rp[l + 1])] = v
    return out


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("fused_steps", [1, 0])
@pytest.mark.parametrize("path", ["joint", "standalone"])
def test_leaf_table(ctx, path, fused_steps, lanes):
    """The 41-leaf table of gp_pred.npz (a COPY and a PREFIX leaf, a leaf without routed rows, four kernel ids) against the
    dense helper fed with download_factor of the same context, within twice the tolerance."""
    T = TABLE
    L = T["kid"].size
    rp, ri, op_, ob = T["route_ptr"], T["route_idx"], T["obs_ptr"], T["obs_idx"]
    ctx.set_option(hipabi.OPT_FUSED_STEPS, fused_steps)
    ctx.set_option(hipabi.OPT_LANES, lanes)
    try:
        _table_setup(ctx)
        if path == "joint":
            ctx.set_test(T["Xt"], rp, ri)
            _, info, _ = ctx.fit()
            ctx.predict_run()
        else:
            _, info, _ = ctx.fit()
            ctx.predict_leaves(T["Xt"], rp, ri)
        assert np.all(info == 0) and ctx.lanes() == lanes
        dmu, dvar = ctx.predict_gradients()
        assert dmu.shape == (int(rp[-1]), T["X"].shape[1])
        rmu, rvar, tmu, tvar = _table_reference(ctx)
        worst = max(float(np.max(np.abs(dmu - rmu) / (2.0 * tmu))), float(np.max(np.abs(dvar - rvar) / (2.0 * tvar))))
        assert worst <= 1.0, worst
        print(f"\ntable {path} fused_steps={fused_steps} lanes={lanes}: worst err/tol {worst:.3g}")
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)


def test_larger_single_gp(ctx):
    """n = 1500, n_t = 400, D = 8, IsoSE: interior tiles."""
    n, nt, D = 1500, 400, 8
    X, y, Xt = dsm.regression_data(n, D, n_test=nt, seed=777)
    c = dict(X=np.asfortranarray(X), y=y, Xt=np.asfortranarray(Xt), mean=float(np.mean(y)), kind=0,
             loghyp=np.array([np.log(0.9), 0.0]), logNoise=float(np.log(0.1)))
    _single(ctx, c, "standalone")
    t_pred = ctx.predict_run()
    dmu, dvar = ctx.predict_gradients()
    _, _, rmu, rvar = _reference(ctx, 0, c)
    tmu, tvar = pgd.tolerances(0, c["loghyp"], c["logNoise"], c["X"], y, c["Xt"], rmu, rvar)
    _check("n1500 dmu", dmu, rmu, 2.0 * tmu)
    _check("n1500 dvar", dvar, rvar, 2.0 * tvar)
    print(f"predict_gradients device seconds {ctx.grad_seconds:.3g} (predict_run {t_pred:.3g})")


def test_failed_leaf_gives_nan_rows(ctx):
    """Leaf 0: a rank-1 linear Gram of size 1e16 (not positive definite in float64, the construction of test_loo_gpu); leaf 1:
    an ordinary IsoSE leaf, whose rows are those of the same leaf fitted alone, to the bit."""
    n0, n1, nt = 140, 100, 9
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Xt = np.linspace(0.05, 0.95, nt).reshape(-1, 1)
    hyp1 = np.array([np.log(0.3), 0.0, np.log(0.1)])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, hyp1)
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    ctx.predict_leaves(Xt, [0, nt, 2 * nt], np.concatenate([np.arange(nt), np.arange(nt)]))
    dmu, dvar = ctx.predict_gradients()
    assert np.all(np.isnan(dmu[:nt])) and np.all(np.isnan(dvar[:nt]))
    c = dict(kind=0, X=np.asfortranarray(X[n0:]), y=y[n0:], Xt=np.asfortranarray(Xt), mean=0.2, loghyp=hyp1[:2], logNoise=hyp1[2])
    _, _, rmu, rvar = _reference(ctx, 1, c)
    tmu, tvar = pgd.tolerances(0, c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], rmu, rvar)
    _check("good leaf dmu", dmu[nt:], rmu, 2.0 * tmu)
    _check("good leaf dvar", dvar[nt:], rvar, 2.0 * tvar)


def test_errors_leave_the_context_usable(ctx):
    c = make_case(0, 40, 16, 2, seed=6400)
    X, y, Xt = c["X"], c["y"], c["Xt"]
    n, nt = X.shape[0], Xt.shape[0]
    hyp = np.concatenate([c["loghyp"], [c["logNoise"]]])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
    ctx.set_hyper(0, 0, hyp)
    ctx.fit()
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    with pytest.raises(hipabi.DsmgpError) as e:         # before predict_run
        ctx.predict_gradients()
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    d = ctx.predict_gradients()
    import ctypes as C
    buf = np.empty((nt, 2), order="F")
    rc = ctx.lib.dsmgp_predict_gradients(ctx.h, buf.ctypes.data_as(C.POINTER(C.c_double)), None, nt - 1, None)     # ld < route_total
    assert rc == hipabi.E_ARG
    assert _same_bits(d[0], ctx.predict_gradients()[0])
    hyp2 = hyp.copy()
    hyp2[0] += 0.1
    ctx.set_hyper(0, 0, hyp2)
    ctx.fit()                                           # a new fit: predict_run has not finished the rows
    with pytest.raises(hipabi.DsmgpError) as e:
        ctx.predict_gradients()
    assert e.value.code == hipabi.E_STATE
    ctx.predict_run()
    d2 = ctx.predict_gradients()
    assert not _same_bits(d[0], d2[0]) and np.all(np.isfinite(d2[0])) and np.all(np.isfinite(d2[1]))


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gpoe", "rbcm", "gp"])
def test_model_api(family):
    """predict_gradients(model, x): (mu, var) are predict's bits; the gradients are the host aggregation of the per-entry
    device outputs (the aggregation itself is checked on the CPU: test_predgrad_host.py)."""
    X, y, Xt = dsm.regression_data(600, 2, n_test=24, seed=99)
    kern = dsm.IsoSE(np.log(0.4), 0.0)
    if family == "dsmgp":
        model = dsm.buildDSMGP(X, y, 2, 3, M=60, kernel=kern, logNoise=np.log(0.1), seed=3)
    elif family in ("poe", "gpoe"):
        model = dsm.buildPoE(X, y, 3, M=60, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), logNoise=np.log(0.1),
                             generalized=family == "gpoe", seed=3)
    elif family == "rbcm":
        model = dsm.buildBCM(X, y, 3, M=60, kernel=kern, logNoise=np.log(0.1), robust=True, seed=3)
    else:
        model = dsm.GaussianProcess(X, y, kernel=kern, logNoise=np.log(0.1), run_cholesky=True)
    if family != "gp":
        dsm.fit(model)
    dsm.predict(model, Xt)      # (registers the rows: the first prediction after a fit runs the standalone sweep, later ones finish
                                #  the moments of COPY / PREFIX leaves from the stored rows -- predict's own bits differ between the two)
    mu, var, dmu, dvar = dsm.predict_gradients(model, Xt)
    mu0, var0 = dsm.predict(model, Xt)
    assert _same_bits(mu, mu0) and _same_bits(var, var0)
    assert dmu.shape == Xt.shape and dvar.shape == Xt.shape and np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
    if family == "gp":
        a, b = model.model.ctx.predict_gradients()
        assert _same_bits(dmu, a) and _same_bits(dvar, b)
        return
    from deepstructuredmixtures_amd import model as dmodel
    from pred_tolerance import row_entries
    rc = dmodel._routing(model, np.asfortranarray(Xt))
    ptr, idx = rc["lptr"], rc["lidx"]
    mu_l, var_l = model.ctx.predict_fetch()
    dmu_l, dvar_l = model.ctx.predict_gradients()
    fam, coef, group, G, plain, prior = dmodel._aggregation_spec(model)
    kw = {}
    if fam == hipabi.AGG_RBCM:
        kw = dict(kss_prior=np.full(Xt.shape[0], np.exp(2 * prior.kernel.logs)), noise_prior=np.exp(2 * prior.logNoise))
    a, b = dsm.aggregate_input_gradients(fam, mu_l, var_l, dmu_l, dvar_l, row_entries(ptr, idx, Xt.shape[0]), coef=coef,
                                         group=group, G=G, plain=plain, **kw)
    assert _same_bits(dmu, a) and _same_bits(dvar, b)
