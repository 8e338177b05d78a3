"""GPU tests of dsmgp_aggregate_gradients*: the input gradients of the aggregated prediction, reduced on the device from the
per-entry gradients (agg_grad_partial_kernel, agg_grad_finish_kernel).

Oracle and tolerance: tests/agg_gradients_cases.py -- dsm.aggregate_input_gradients on the same context's predict_fetch() and
predict_gradients(), within twice the rounding bound test_predgrad_host.py derives for that function.  The exact properties
(a repeated call, a row listed twice, dmu alone, what other entry points return before and after) are checked on bits."""
import ctypes as C

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi
import agg_gradients_cases as ac
from test_predcov_gpu import TABLE, _same_bits, _table_setup

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _table_specs():
    T = TABLE
    L = T["kid"].size
    return dict(mixture=ac.spec(ac.MIXTURE, coef=T["w_mix"]), plain=ac.spec(ac.MIXTURE, coef=T["w_mix"], plain=True),
                poe=ac.spec(ac.POE, coef=np.ones(L)), gpoe=ac.spec(ac.GPOE, coef=T["beta"]),
                rbcm=ac.spec(ac.RBCM, group=T["group"], G=int(T["G"]), prior_kid=int(T["prior_kid"])))


def _table_prior():
    T = TABLE
    k = int(T["prior_kid"])
    hyp = T["hyp"][k][:T["hyp_len"][k]]
    return int(T["kinds"][k]), hyp[:-1], float(hyp[-1])


def _table_predict(c, path):
    T = TABLE
    _table_setup(c)
    if path == "joint":
        c.set_test(T["Xt"], T["route_ptr"], T["route_idx"])
        _, info, _ = c.fit()
    else:
        _, info, _ = c.fit()
        c.set_test(T["Xt"], T["route_ptr"], T["route_idx"])
    assert np.all(info == 0)
    c.predict_run()


def _bits(*arrays):
    return [np.array(a, copy=True) for group in arrays for a in (group if isinstance(group, tuple) else (group,)) if a is not None]


def _all_same(a, b):
    return len(a) == len(b) and all(_same_bits(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------ the 41-leaf table

@pytest.mark.parametrize("path", ["joint", "standalone"])
@pytest.mark.parametrize("name", ["mixture", "plain", "poe", "gpoe", "rbcm"])
def test_leaf_table(ctx, name, path):
    """The 41-leaf table of gp_pred.npz (a COPY and a PREFIX leaf, a leaf without routed rows, four kernel ids; the rBCM prior is
    its ArdLinear id, ds/dx != 0) by both routes to K_tn L^-T: the values within tolerance of the host function on the context's own
    per-entry arrays; the same bits from a repeated call, from the call that makes the per-entry gradients itself, and for dmu
    alone; predict_fetch, predict_gradients, aggregate and scores the same bits before and after."""
    T = TABLE
    s = _table_specs()[name]
    _table_predict(ctx, path)
    entries = ac.context_entries(ctx)                   # (leaves both halves of the per-entry gradients current)
    before = _bits(entries, ac.device_moments(ctx, s), tuple(ctx.scores(T["yt"]).values()))
    dmu, dvar = ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
    assert dmu.shape == T["Xt"].shape and dvar.shape == T["Xt"].shape and dmu.flags.f_contiguous
    rm, rv, tm, tv = ac.oracle(s, entries, T["Xt"], T["route_ptr"], T["route_idx"], _table_prior())
    assert np.all(np.isfinite(rm)) and np.all(np.isfinite(rv)) and np.any(rm != 0.0) and np.any(rv != 0.0)
    ac.check(f"table {name} {path} dmu", dmu, rm, tm)
    ac.check(f"table {name} {path} dvar", dvar, rv, tv)
    again = ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
    alone = ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"], want_var=False)
    assert _same_bits(dmu, again[0]) and _same_bits(dvar, again[1]) and _same_bits(dmu, alone[0]) and alone[1] is None
    after = _bits(ac.context_entries(ctx), ctx.aggregate_finish(plain=s["plain"], prior_kernel_id=s["prior_kid"]),
                  tuple(ctx.scores(T["yt"]).values()))
    assert _all_same(before, after)
    # a fresh prediction: the call makes the per-entry gradients itself (no predict_gradients before it), also after a
    # mean-only predict_gradients, which leaves the variance half as it was
    ctx.predict_run()
    own = ac.device_gradients(ctx, s)
    assert _same_bits(dmu, own[0]) and _same_bits(dvar, own[1])
    ctx.predict_run()
    ctx.predict_gradients(want_var=False)
    own = ac.device_gradients(ctx, s)
    assert _same_bits(dmu, own[0]) and _same_bits(dvar, own[1])
    assert _all_same(before[:4], _bits(ac.context_entries(ctx)))


# ------------------------------------------------------------------------------------------ shapes of the row kernel

@pytest.mark.parametrize("name", ["mixture", "plain", "poe", "gpoe", "rbcm"])
@pytest.mark.parametrize("n_t,D", [(1, 3), (255, 1), (257, 3), (257, 40), (257, 8), (257, 9), (70, 17)])
def test_shapes(ctx, n_t, D, name):
    """n_t on both sides of the 256-thread block, D = 1, 3, 40 and, around the chunk of 8 dimensions the kernels work in, D = 8
    (exactly one chunk), 9 (a tail of one) and 17 (three rounds); rows with no, one and up to six entries; G = 3 groups of which
    some rows see one or two; the rBCM prior is the ArdLinear id.  A row without entries gets what the formulas give (NaN for
    the products, 0 and ds/dx for the others), as the host function does."""
    t = ac.small_table(n_t, D, 9100 + n_t + D)
    s = t["specs"][name]
    ac.small_predict(ctx, t)
    entries = ac.context_entries(ctx)
    dmu, dvar = ac.device_gradients(ctx, s)
    assert dmu.shape == (n_t, D)
    rm, rv, tm, tv = ac.oracle(s, entries, t["Xt"], t["route_ptr"], t["route_idx"], t["prior"])
    counts = np.bincount(t["route_idx"], minlength=n_t)
    if n_t > 2:
        assert counts.min() == 0 and 1 in counts and counts.max() == ac.N_LEAVES
    if name in ("poe", "gpoe"):
        assert np.all(np.isnan(rm[counts == 0])) and np.all(np.isfinite(rm[counts > 0]))
    else:
        assert np.all(np.isfinite(rm)) and np.all(np.isfinite(rv))
    if name == "rbcm" and n_t > 2:
        groups = [{int(g) for g in s["group"][[l for l in range(ac.N_LEAVES) if r in
                                                t["route_idx"][t["route_ptr"][l]:t["route_ptr"][l + 1]]]]} for r in range(n_t)]
        assert any(len(g) == 2 for g in groups) and any(len(g) == 1 for g in groups) and any(len(g) == 3 for g in groups)
        assert np.any(rv[counts == 0] != 0.0)           # ds/dx of the linear prior alone
    ac.check(f"shape {n_t}x{D} {name} dmu", dmu, rm, tm)
    ac.check(f"shape {n_t}x{D} {name} dvar", dvar, rv, tv)


def test_a_row_listed_twice_gets_identical_rows(ctx):
    """The last test row is a copy of row 3 (which reaches every leaf), routed to the same leaves: identical bits, every family."""
    t = ac.small_table(40, 3, 9300)
    n_t = 41
    Xt = np.asfortranarray(np.vstack([t["Xt"], t["Xt"][3:4]]))
    rp, ri = t["route_ptr"], t["route_idx"]
    lists = [ri[rp[l]:rp[l + 1]].tolist() for l in range(ac.N_LEAVES)]
    lists = [v + [40] if 3 in v else v for v in lists]
    assert all(40 in v for v in lists)
    ac.small_setup(ctx, t)
    ctx.fit()
    ctx.set_test(Xt, np.concatenate([[0], np.cumsum([len(v) for v in lists])]), np.array([r for v in lists for r in v]))
    ctx.predict_run()
    for name, s in t["specs"].items():
        dmu, dvar = ac.device_gradients(ctx, s)
        assert dmu.shape == (n_t, 3) and np.all(np.isfinite(dmu[3])) and np.any(dmu[3] != 0.0)
        assert _same_bits(dmu[3], dmu[40]) and _same_bits(dvar[3], dvar[40]), name


# ------------------------------------------------------------------------------------------ clamp, failed leaf

def test_clamped_leaf_variance_is_a_constant(ctx):
    """An IsoLinear leaf, n = 40, D = 1, logNoise = -30, 64 test rows at training rows: the leaf variance is rounding of either
    sign.  Where predict_fetch shows var <= 0 the mixture result is the host function's, which zeroes that dvar_l.
    The inputs are of size 1e3: with the rank-one Gram x x' / l^2 and K_y = K + d I, d = 1e-8 (the factorisation's jitter; the
    noise is 1e-26), the exact variance at a training row is x^2 d / (sum x^2 + d) ~ 1e6 1e-8 / 1e8 = 1e-10, and it is formed
    as the difference of k** and |L^-1 k*|^2, both ~ 1e6 and each rounded at eps 1e6 = 2e-10.  (Inputs of size 1 give
    variances of 1e-11 .. 1e-10 against a rounding of 1e-16: all positive.)"""
    n, nt = 40, 64
    X = np.linspace(500.0, 2500.0, n).reshape(-1, 1)
    y = 0.8e-3 * X[:, 0] + 0.05 * np.sin(0.04 * X[:, 0])
    Xt = np.asfortranarray(X[np.arange(nt) % n])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    _, info, _ = ctx.fit()
    assert info[0] == 0
    ctx.set_test(Xt, [0, nt], np.arange(nt))
    ctx.predict_run()
    entries = ac.context_entries(ctx)
    clamped = ~(entries[1] > 0)
    print(f"\nclamp: {int(clamped.sum())} of {nt} leaf variances <= 0, min {entries[1].min():.3g} max {entries[1].max():.3g}")
    assert clamped.any(), "no leaf variance came out <= 0: the case shows nothing"
    for plain in (False, True):
        s = ac.spec(ac.MIXTURE, coef=[1.0], plain=plain)
        dmu, dvar = ac.device_gradients(ctx, s)
        rm, rv, tm, tv = ac.oracle(s, entries, Xt, [0, nt], np.arange(nt))
        ac.check(f"clamp plain={plain} dmu", dmu, rm, tm)
        ac.check(f"clamp plain={plain} dvar", dvar, rv, tv)
        if plain:
            assert np.all(dvar[clamped] == 0.0) and np.all(rv[clamped] == 0.0)


def test_failed_leaf_gives_nan_rows(ctx):
    """The construction of test_predgrad_gpu.test_failed_leaf_gives_nan_rows, with rows 0 .. 5 routed to both leaves and rows
    6 .. 8 to the healthy leaf alone: the first six rows are NaN, the others finite and within tolerance, every family."""
    n0, n1, nt = 140, 100, 9
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Xt = np.asfortranarray(np.linspace(0.05, 0.95, nt).reshape(-1, 1))
    hyp1 = np.array([np.log(0.3), 0.0, np.log(0.1)])
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, hyp1)
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    rp, ri = np.array([0, 6, 6 + nt]), np.concatenate([np.arange(6), np.arange(nt)])
    ctx.set_test(Xt, rp, ri)
    ctx.predict_run()
    entries = ac.context_entries(ctx)
    good = np.arange(nt) >= 6
    specs = dict(mixture=ac.spec(ac.MIXTURE, coef=[0.4, 0.6]), plain=ac.spec(ac.MIXTURE, coef=[0.4, 0.6], plain=True), poe=ac.spec(ac.POE, coef=[1.0, 1.0]), gpoe=ac.spec(ac.GPOE, coef=[0.5, 0.5]),
                 rbcm=ac.spec(ac.RBCM, group=[0, 1], G=2, prior_kid=1))
    for name, s in specs.items():
        dmu, dvar = ac.device_gradients(ctx, s)
        assert np.all(np.isnan(dmu[~good])) and np.all(np.isnan(dvar[~good])), name
        assert np.all(np.isfinite(dmu[good])) and np.all(np.isfinite(dvar[good])), name
        rm, rv, tm, tv = ac.oracle(s, entries, Xt, rp, ri, (0, hyp1[:2], hyp1[2]))
        ac.check(f"failed leaf {name} dmu", dmu, rm, tm, rows=good)
        ac.check(f"failed leaf {name} dvar", dvar, rv, tv, rows=good)


# ------------------------------------------------------------------------------------------ the split over contexts

def _mc_entries(mc):
    return mc.predict_fetch() + mc.predict_gradients()


def _pair(fused_steps):
    """The 41-leaf table predicted on a single context and on MultiContext(0, n=2), one lane each: (single, mc, the entries of each)."""
    T = TABLE
    one, mc = hipabi.Context(0), hipabi.MultiContext(0, n=2)
    try:
        for c in (one, mc):
            c.set_option(hipabi.OPT_LANES, 1)
            c.set_option(hipabi.OPT_FUSED_STEPS, fused_steps)
            _table_setup(c)
            c.fit()
            c.set_test(T["Xt"], T["route_ptr"], T["route_idx"])
            c.predict_run()
        with pytest.raises(hipabi.DsmgpError) as e:
            mc.aggregate_gradients()                    # before aggregate_partial
        assert e.value.code == hipabi.E_STATE
        yield one, mc, ac.context_entries(one), _mc_entries(mc)
    finally:
        mc.close()
        one.close()


@pytest.fixture(scope="module")
def two():
    yield from _pair(1)


@pytest.fixture(scope="module")
def two_classic():
    yield from _pair(0)


@pytest.mark.parametrize("name", ["mixture", "plain", "poe", "gpoe", "rbcm"])
def test_split_over_two_contexts(two, name):
    """MultiContext(0, n=2): total moments to every sub-context, gradient sums added in context order, finish on the first.
    Within tolerance of the host function on the MultiContext's own per-entry arrays."""
    T = TABLE
    _, mc, _, entries = two
    s = _table_specs()[name]
    mc.aggregate_partial(s["family"], s["coef"], s["group"], s["G"])
    dmu, dvar = mc.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
    rm, rv, tm, tv = ac.oracle(s, entries, T["Xt"], T["route_ptr"], T["route_idx"], _table_prior())
    ac.check(f"split {name} dmu", dmu, rm, tm)
    ac.check(f"split {name} dvar", dvar, rv, tv)
    again = mc.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
    assert _same_bits(dmu, again[0]) and _same_bits(dvar, again[1])


def test_split_agrees_with_the_single_context(two_classic, two):
    """MultiContext(0, n=2) against the single context within twice the tolerance, every family.  The tolerance is that of the
    aggregation given its inputs, so the comparison needs two contexts whose per-entry inputs agree, and it is made where they
    do, to the bit: with the shallow block steps not fused (OPT_FUSED_STEPS = 0, the setting test_leaf_table of the per-entry
    tests runs beside the default).  With the default the plan chooses its fused steps by the number of leaves it holds, a
    context with half of the table chooses otherwise than one with all of it, and every leaf's factor, moments and gradients
    differ between the two in their last bits times cond(K_y) (measured on an MI355X: up to 5e-13 in mu and 4e-13 in dmu per
    entry; test_predgrad_gpu.test_multicontext_puts_the_entries_back_in_order bounds that by the per-entry tolerance).  That
    difference is no property of the split: under the default the test prints what it does to the aggregate; each side
    against its own entries is test_leaf_table and test_split_over_two_contexts."""
    T = TABLE
    one, mc, e_one, e_mc = two_classic
    assert all(_same_bits(a, b) for a, b in zip(e_one, e_mc)), "the per-entry inputs of the two contexts differ: nothing to compare"
    worst = {}
    for name, s in _table_specs().items():
        single = ac.device_gradients(one, s)
        mc.aggregate_partial(s["family"], s["coef"], s["group"], s["G"])
        split = mc.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
        _, _, tm, tv = ac.oracle(s, e_mc, T["Xt"], T["route_ptr"], T["route_idx"], _table_prior())
        worst[name] = max(float(np.max(np.abs(split[0] - single[0]) / (2.0 * tm))), float(np.max(np.abs(split[1] - single[1]) / (2.0 * tv))))
        print(f"\nsplit against single, {name}: |difference| / (2 tol) {worst[name]:.3g}")
    assert all(v <= 1.0 for v in worst.values()), worst
    d_one, d_mc, f_one, f_mc = two
    s = _table_specs()["mixture"]
    single = ac.device_gradients(d_one, s)
    d_mc.aggregate_partial(s["family"], s["coef"], s["group"], s["G"])
    split = d_mc.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
    print(f"default options: per-entry dmu differs by up to {float(np.max(np.abs(f_one[2] - f_mc[2]))):.3g}, the mixture's aggregated dmu by "
          f"{float(np.max(np.abs(split[0] - single[0]))):.3g}")


def test_partial_handed_back_gives_the_bits_of_the_one_call_form(ctx):
    t = ac.small_table(257, 3, 9400)
    ac.small_predict(ctx, t)
    for name, s in t["specs"].items():
        one = ac.device_gradients(ctx, s)
        part = ctx.aggregate_gradients_partial()
        assert part.shape == (hipabi.agg_gradients_width(s["family"], s["G"], 3), 257)
        own = ctx.aggregate_gradients_finish(None, plain=s["plain"], prior_kernel_id=s["prior_kid"])
        back = ctx.aggregate_gradients_finish(part, plain=s["plain"], prior_kernel_id=s["prior_kid"])
        for got in (own, back):
            assert _same_bits(one[0], got[0]) and _same_bits(one[1], got[1]), name
        assert ctx.aggregate_gradients_partial(fetch=False) is None and _same_bits(part, ctx.aggregate_gradients_partial())


# ------------------------------------------------------------------------------------------ states and arguments

def _code(fn, *a, **kw):
    with pytest.raises(hipabi.DsmgpError) as e:
        fn(*a, **kw)
    return e.value.code


def test_states_and_arguments_leave_the_context_usable(ctx):
    t = ac.small_table(40, 3, 9500)
    s, r = t["specs"]["mixture"], t["specs"]["rbcm"]
    ac.small_predict(ctx, t)
    # before aggregate; before aggregate_gradients_partial
    assert _code(ctx.aggregate_gradients) == hipabi.E_STATE and _code(ctx.aggregate_gradients_partial) == hipabi.E_STATE
    ctx.aggregate_partial(s["family"], s["coef"])
    assert _code(ctx.aggregate_gradients) == hipabi.E_STATE                      # sums, but no aggregated moments yet
    ctx.aggregate_finish()
    assert _code(ctx.aggregate_gradients_finish) == hipabi.E_STATE
    good = ctx.aggregate_gradients()
    # ld < n_t, on the one-call form and on finish; then a bad rBCM prior id
    buf = np.empty((40, 3), order="F")
    assert ctx.lib.dsmgp_aggregate_gradients(ctx.h, 0, 0, buf.ctypes.data_as(_dp), None, 39, None) == hipabi.E_ARG
    assert ctx.lib.dsmgp_aggregate_gradients_finish(ctx.h, None, 0, 0, buf.ctypes.data_as(_dp), None, 39) == hipabi.E_ARG
    assert ctx.lib.dsmgp_aggregate_gradients(ctx.h, 0, 0, buf.ctypes.data_as(_dp), None, 40, None) == 0
    assert _same_bits(buf, good[0])
    ac.device_moments(ctx, r, fetch=False)
    assert _code(ctx.aggregate_gradients, prior_kernel_id=7) == hipabi.E_ARG and _code(ctx.aggregate_gradients, prior_kernel_id=-1) == hipabi.E_ARG
    rb = ctx.aggregate_gradients(prior_kernel_id=r["prior_kid"])
    assert np.all(np.isfinite(rb[0][np.bincount(t["route_idx"], minlength=40) > 0]))
    # new moments fell the gradient sums; so do new hyper-parameters and a new fit
    ac.device_moments(ctx, s, fetch=False)
    assert _code(ctx.aggregate_gradients_finish) == hipabi.E_STATE
    again = ctx.aggregate_gradients()
    assert _same_bits(good[0], again[0]) and _same_bits(good[1], again[1])
    kind, hyp = t["hyp"][ac.KID_SE]
    hyp2 = hyp.copy()
    hyp2[0] += 0.1
    ctx.set_hyper(ac.KID_SE, kind, hyp2)
    assert _code(ctx.aggregate_gradients) == hipabi.E_STATE and _code(ctx.aggregate_gradients_finish) == hipabi.E_STATE
    ctx.fit()
    assert _code(ctx.aggregate_gradients) == hipabi.E_STATE
    ctx.predict_run()
    assert _code(ctx.aggregate_gradients) == hipabi.E_STATE                      # the moments of the new prediction are not aggregated yet
    new = ac.device_gradients(ctx, s)
    assert not _same_bits(good[0], new[0])
    rm, rv, tm, tv = ac.oracle(s, ac.context_entries(ctx), t["Xt"], t["route_ptr"], t["route_idx"])
    ac.check("after a new fit dmu", new[0], rm, tm)
    ac.check("after a new fit dvar", new[1], rv, tv)


# ------------------------------------------------------------------------------------------ the model functions

def _model(family, **kw):
    X, y, Xt = dsm.regression_data(600, 2, n_test=24, seed=99)
    kern = dsm.IsoSE(np.log(0.4), 0.0)
    if family == "dsmgp":
        model = dsm.buildDSMGP(X, y, 2, 3, M=60, kernel=kern, logNoise=np.log(0.1), seed=3, **kw)
    elif family in ("poe", "gpoe"):
        model = dsm.buildPoE(X, y, 3, M=60, kernel=kern, meanFun=dsm.ConstMean(float(np.mean(y))), logNoise=np.log(0.1),
                             generalized=family == "gpoe", seed=3, **kw)
    elif family == "rbcm":
        model = dsm.buildBCM(X, y, 3, M=60, kernel=kern, logNoise=np.log(0.1), robust=True, seed=3, **kw)
    else:
        model = dsm.GaussianProcess(X, y, kernel=kern, logNoise=np.log(0.1), run_cholesky=True)
    if family != "gp":
        dsm.fit(model)
    return model, Xt


def _model_tolerance(model, Xt, family):
    """The tolerance of the device aggregate for a model: the oracle on the model context's own per-entry arrays."""
    from deepstructuredmixtures_amd import model as dmodel
    target = model.model if family == "gp" else model
    xt = np.asfortranarray(Xt)
    rc = dmodel._routing(target, xt)
    fam, coef, group, G, plain, prior = dmodel._aggregation_spec(target)
    s = ac.spec(fam, coef=coef, group=group, G=G, plain=plain, prior_kid=prior.kernelid if prior else 0)
    pr = (0, np.array([prior.kernel.logl, prior.kernel.logs], dtype=np.float64).ravel(), prior.logNoise) if prior else None
    entries = target.ctx.predict_fetch() + target.ctx.predict_gradients()
    return ac.oracle(s, entries, xt, rc["lptr"], rc["lidx"], pr)


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gpoe", "rbcm", "gp"])
def test_model_api(family):
    """predict_gradients(model, x, aggregate="device"): (mu, var) are predict's bits, the gradients within tolerance of the
    host aggregation; the default is the host aggregation (its bits are pinned by test_predgrad_gpu.test_model_api)."""
    model, Xt = _model(family)
    dsm.predict(model, Xt)
    mu, var, dmu, dvar = dsm.predict_gradients(model, Xt, aggregate="device")
    mu0, var0 = dsm.predict(model, Xt)
    assert _same_bits(mu, mu0) and _same_bits(var, var0)
    assert dmu.shape == Xt.shape and dvar.shape == Xt.shape and np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
    hm, hv, hdmu, hdvar = dsm.predict_gradients(model, Xt, aggregate="host")
    dm, dv, ddmu, ddvar = dsm.predict_gradients(model, Xt)
    assert _same_bits(hm, mu) and _same_bits(hv, var) and _same_bits(hdmu, ddmu) and _same_bits(hdvar, ddvar)
    _, _, tm, tv = _model_tolerance(model, Xt, family)
    ac.check(f"model {family} dmu", dmu, hdmu, tm)
    ac.check(f"model {family} dvar", dvar, hdvar, tv)
    with pytest.raises(ValueError, match="aggregate must be"):
        dsm.predict_gradients(model, Xt, aggregate="gpu")


def test_model_on_two_contexts():
    """A DSMGP on a MultiContext: aggregate="device" goes through the split and agrees with the host aggregation."""
    model, Xt = _model("dsmgp", n_sub=2)
    assert isinstance(model.ctx, hipabi.MultiContext)
    mu, var, dmu, dvar = dsm.predict_gradients(model, Xt, aggregate="device")
    hm, hv, hdmu, hdvar = dsm.predict_gradients(model, Xt)
    assert _same_bits(mu, hm) and _same_bits(var, hv)
    _, _, tm, tv = _model_tolerance(model, Xt, "dsmgp")
    ac.check("model on two contexts dmu", dmu, hdmu, tm)
    ac.check("model on two contexts dvar", dvar, hdvar, tv)


# ------------------------------------------------------------------------------------------ the target columns

def _columns(t, Q, seed=5):
    """(Y, mean): Q columns over the small table's training rows, column 0 the table's own y; the leaf means of every column."""
    rng = np.random.default_rng(seed)
    Y = t["y"][:, None] * (1.0 + 0.3 * np.arange(Q))[None, :] + np.where(np.arange(Q) > 0, 0.2, 0.0)[None, :] * rng.standard_normal((t["y"].size, Q))
    op, oi = t["obs_ptr"], t["obs_idx"]
    mean = np.stack([np.mean(Y[oi[op[l]:op[l + 1]]], axis=0) for l in range(ac.N_LEAVES)])
    mean[:, 0] = t["mean"]
    return np.asfortranarray(Y), mean


def _device_columns(ctx, s):
    mu, var = ctx.aggregate_columns(s["family"], s["coef"], s["group"], s["G"], plain=s["plain"], prior_kernel_id=s["prior_kid"])
    dmu, dvar = ctx.aggregate_columns_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
    return mu, var, dmu, dvar


def _columns_against_the_host(ctx, Q, n_t, D, seed):
    t = ac.small_table(n_t, D, seed)
    Y, mean = _columns(t, Q)
    ac.small_predict(ctx, t)
    ctx.solve_targets(Y, mean)
    counts = np.bincount(t["route_idx"], minlength=n_t)
    some = counts > 0
    assert not some.all()
    for name, s in t["specs"].items():
        single = ac.device_moments(ctx, s)
        ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
        yt = np.linspace(0.0, 1.0, n_t)
        before = _bits(single, ctx.aggregate_gradients_finish(plain=s["plain"], prior_kernel_id=s["prior_kid"]), tuple(ctx.scores(yt).values()))
        mu, var, dmu, dvar = _device_columns(ctx, s)
        assert mu.shape == (n_t, Q) and dvar.shape == (n_t, D, Q)
        (rm, rv, tm, tv), (gm, gv, tgm, tgv) = ac.columns_oracle(ctx, s, t["Xt"], t["route_ptr"], t["route_idx"], t["prior"])
        ac.check(f"columns Q={Q} {name} mu", mu, rm, tm, rows=some)
        ac.check(f"columns Q={Q} {name} var", var, rv, tv, rows=some)
        ac.check(f"columns Q={Q} {name} dmu", dmu, gm, tgm)
        ac.check(f"columns Q={Q} {name} dvar", dvar, gv, tgv)
        for q in range(Q):      # rows without entries: what dsmgp_aggregate gives them
            assert np.array_equal(mu[~some, q], single[0][~some], equal_nan=True) and np.array_equal(var[~some, q], single[1][~some], equal_nan=True)
        if name != "mixture" and Q > 1:     # the leaf variance is shared: only the mixture's variance depends on the column
            assert _same_bits(var[:, 0], var[:, Q - 1]) and _same_bits(dvar[:, :, 0], dvar[:, :, Q - 1])
        again = _device_columns(ctx, s)     # (the per-entry arrays are current now: read as they are)
        assert all(_same_bits(a, b) for a, b in zip((mu, var, dmu, dvar), again))
        after = _bits(ctx.aggregate_finish(plain=s["plain"], prior_kernel_id=s["prior_kid"]),
                      ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"]), tuple(ctx.scores(yt).values()))
        assert _all_same(before, after), name


@pytest.mark.parametrize("Q", [1, 3, 17])
def test_columns_against_the_host(ctx, Q):
    """Q = 1, 3, 17 (across Qpad = 16), every family, column by column: the moments within twice agg_tol of
    pred_tolerance.aggregate, the gradients within tolerance of the host function, both on the context's own per-entry arrays;
    rows without entries as dsmgp_aggregate gives them; a repeated call the same bits; and the single-y state (aggregate_finish,
    aggregate_gradients_finish, scores) the same bits before and after."""
    _columns_against_the_host(ctx, Q, 70, 3, 9600)


def test_columns_against_the_host_past_one_chunk_of_dimensions(ctx):
    """The same checks at D = 9, Q = 3: agg_columns_grad_kernel works in chunks of 8 dimensions, so a second round with a tail
    of one."""
    _columns_against_the_host(ctx, 3, 70, 9, 9650)


def test_one_column_of_y_equals_the_single_y_calls(ctx):
    """Y = y[:, None] with the leaf means: the column calls against dsmgp_aggregate and dsmgp_aggregate_gradients.  The per-entry
    means and their gradients come from other kernels than the single-y ones (a tile product on the matrix cores), so they agree
    within the per-entry tolerances of the prediction tests (pred_tolerance.moment_tol, predgrad_dense.tolerances) and not to
    4 eps; the bound carries THOSE through the aggregation (Prop), doubled.  The shared variances are the same arrays: 4 eps."""
    from pred_tolerance import moment_tol
    import predgrad_dense as pgd
    n_t, D = 70, 3
    t = ac.small_table(n_t, D, 9700)
    ac.small_predict(ctx, t)
    ctx.solve_targets(t["y"][:, None], t["mean"][:, None])
    mu_l, var_l, dmu_l, dvar_l = ac.context_entries(ctx)
    rp, ri, op, oi = t["route_ptr"], t["route_idx"], t["obs_ptr"], t["obs_idx"]
    yscale = max(1.0, float(np.max(np.abs(t["y"]))))
    tol_mu = moment_tol(mu_l, var_l, np.ones_like(mu_l), 0.0, yscale)[0]
    tol_dmu = np.zeros_like(dmu_l)
    for l in range(ac.N_LEAVES):
        kind, hyp = t["hyp"][int(t["kid"][l])]
        e = slice(int(rp[l]), int(rp[l + 1]))
        obs = oi[op[l]:op[l + 1]]
        tol_dmu[e] = pgd.tolerances(kind, hyp[:-1], hyp[-1], t["X"][obs], t["y"][obs], t["Xt"][ri[e]], dmu_l[e], dvar_l[e])[0]
    etol = (tol_mu, 4 * ac.EPS * np.abs(var_l), tol_dmu, 4 * ac.EPS * np.abs(dvar_l))
    some = np.bincount(ri, minlength=n_t) > 0
    for name, s in t["specs"].items():
        m1, v1 = ac.device_moments(ctx, s)
        g1 = ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"])
        mu, var, dmu, dvar = _device_columns(ctx, s)
        _, _, tm, tv = ac.moments_oracle(s, mu_l, var_l, t["Xt"], rp, ri, t["prior"], tol_mu=tol_mu)
        _, _, tgm, tgv = ac.oracle(s, (mu_l, var_l, dmu_l, dvar_l), t["Xt"], rp, ri, t["prior"], entry_tol=etol)
        ac.check(f"one column {name} mu", mu[:, 0], m1, tm, rows=some)
        ac.check(f"one column {name} var", var[:, 0], v1, tv, rows=some)
        ac.check(f"one column {name} dmu", dmu[:, :, 0], g1[0], tgm)
        ac.check(f"one column {name} dvar", dvar[:, :, 0], g1[1], tgv)


def test_a_column_does_not_depend_on_the_others(ctx):
    """Column q is the same bits at Q = 3 and at Q = 17, and with the other columns replaced."""
    t = ac.small_table(70, 3, 9800)
    Y17, m17 = _columns(t, 17)
    Yr, mr = Y17[:, :3].copy(order="F"), m17[:, :3].copy()
    Yr[:, 1:] = np.cos(7.0 * Yr[:, 1:]) * 3.0
    ac.small_predict(ctx, t)
    got = {}
    for key, (Y, m) in dict(q17=(Y17, m17), q3=(np.asfortranarray(Y17[:, :3]), m17[:, :3]), other=(Yr, mr)).items():
        ctx.solve_targets(Y, m)
        got[key] = {name: _device_columns(ctx, s) for name, s in t["specs"].items()}
    for name in t["specs"]:
        for a, b in zip(got["q3"][name], got["q17"][name]):
            assert _same_bits(a[..., :3], b[..., :3]), name
        for a, b in zip(got["q3"][name], got["other"][name]):
            assert _same_bits(a[..., 0], b[..., 0]), name
        assert not _same_bits(got["q3"][name][0][..., 1], got["other"][name][0][..., 1])


def test_column_states_and_arguments(ctx):
    t = ac.small_table(40, 3, 9900)
    s, r = t["specs"]["mixture"], t["specs"]["rbcm"]
    Y, mean = _columns(t, 3)
    ac.small_predict(ctx, t)
    args = (s["family"], s["coef"])
    assert _code(ctx.aggregate_columns, *args) == hipabi.E_STATE                    # before solve_targets
    assert _code(ctx.aggregate_columns_gradients) == hipabi.E_STATE
    ctx.solve_targets(Y, mean)
    assert _code(ctx.aggregate_columns_gradients) == hipabi.E_STATE                 # before aggregate_columns
    good = ctx.aggregate_columns(*args) + ctx.aggregate_columns_gradients()
    buf = np.empty((40, 9), order="F")
    p = buf.ctypes.data_as(_dp)
    coef = np.ascontiguousarray(s["coef"])
    assert ctx.lib.dsmgp_aggregate_columns(ctx.h, 0, coef.ctypes.data_as(_dp), None, 0, 0, 0, p, None, 39, None) == hipabi.E_ARG
    assert ctx.lib.dsmgp_aggregate_columns_gradients(ctx.h, 0, 0, p, None, 39, None) == hipabi.E_ARG
    assert ctx.lib.dsmgp_aggregate_columns_gradients(ctx.h, 0, 0, p, None, 40, None) == 0 and _same_bits(buf.reshape((40, 3, 3), order="F"), good[2])
    assert _code(ctx.aggregate_columns, r["family"], None, r["group"], r["G"], prior_kernel_id=7) == hipabi.E_ARG
    assert _code(ctx.aggregate_columns, 9, s["coef"]) == hipabi.E_ARG
    again = ctx.aggregate_columns(*args) + ctx.aggregate_columns_gradients()
    assert all(_same_bits(a, b) for a, b in zip(good, again))
    ctx.solve_targets(Y[:, :2], mean[:, :2])                                        # new columns fell the column moments
    assert _code(ctx.aggregate_columns_gradients) == hipabi.E_STATE
    ctx.aggregate_columns(*args)
    ctx.predict_run()                                                               # ... and so does a new prediction
    assert _code(ctx.aggregate_columns_gradients) == hipabi.E_STATE
    ctx.fit()
    assert _code(ctx.aggregate_columns, *args) == hipabi.E_STATE
    mc = hipabi.MultiContext.__new__(hipabi.MultiContext)
    assert not hasattr(mc, "aggregate_columns")


@pytest.mark.parametrize("family", ["dsmgp", "poe", "gpoe", "rbcm", "gp"])
def test_model_api_columns(family):
    """predict_targets / predict_targets_gradients with aggregate="device" within tolerance of aggregate="host" (the default,
    whose bits the existing column tests pin), Q = 3."""
    model, Xt = _model(family)
    target = model.model if family == "gp" else model
    Y = np.stack([target.y, np.cos(3.0 * target.x[:, 0]), target.y ** 2], axis=1)
    dsm.fit_targets(model, Y)
    hm, hv, hdm, hdv = dsm.predict_targets_gradients(model, Xt)
    dm, dv = dsm.predict_targets(model, Xt, aggregate="device")
    mu, var, dmu, dvar = dsm.predict_targets_gradients(model, Xt, aggregate="device")
    assert _same_bits(dm, mu) and _same_bits(dv, var) and mu.shape == (24, 3) and dmu.shape == (24, 3, 2)
    from deepstructuredmixtures_amd import model as dmodel
    xt = np.asfortranarray(Xt)
    rc = dmodel._routing(target, xt)
    fam, coef, group, G, plain, prior = dmodel._aggregation_spec(target)
    s = ac.spec(fam, coef=coef, group=group, G=G, plain=plain, prior_kid=prior.kernelid if prior else 0)
    pr = (0, np.array([prior.kernel.logl, prior.kernel.logs]), prior.logNoise) if prior else None
    (_, _, tm, tv), (_, _, tgm, tgv) = ac.columns_oracle(target.ctx, s, xt, rc["lptr"], rc["lidx"], pr)
    ac.check(f"model columns {family} mu", mu, hm, tm)
    ac.check(f"model columns {family} var", var, hv, tv)
    ac.check(f"model columns {family} dmu", dmu, hdm, tgm.transpose(0, 2, 1))
    ac.check(f"model columns {family} dvar", dvar, hdv, tgv.transpose(0, 2, 1))
    with pytest.raises(ValueError, match="aggregate must be"):
        dsm.predict_targets(model, Xt, aggregate="gpu")
