"""GPU tests of dsmgp_add_rows_keep_test: the resident test set stays across appended rows and dsmgp_predict_run resumes K_tn L^-T
from the block columns the call kept.

Context a: old fit, set_test, predict_run, append_rows(keep_test=True), predict_run.  Context b: the grown table from scratch,
set_test, predict_run.  Routes (host): seven_leaves -- a 150-row test matrix, leaf l takes rows arange(c_l) with c = [150, 40, 1,
130, 17, 40, 0] (two row tiles with a 2-row and a 22-row tail, one row, no rows; the COPY leaf has routes of its own; the 730-row
leaf reaches classic steps with K > 512); many_small_leaves -- 20 rows per leaf (fused steps).

Tolerances are the project's: the factor side as tests/test_append_gpu.py (_compare_with_scratch); moments of a against b within
pred_tolerance.moment_tol; against the dense reference of the grown leaf rtol 1e-8 with atol 1e-9 (mu) / 1e-10 (var), as
tests/test_gpu_parity.py; predict_cov within test_predcov_gpu.entry_tol; predict_gradients within twice predgrad_dense.tolerances
(two float64 results, as test_predgrad_gpu compares two contexts); predict_targets within targets_dense.mu_tol; the PoE aggregate
within pred_tolerance.agg_tol."""
import numpy as np
import pytest

import append_tables as at
import deepstructuredmixtures_amd as dsm
import dense_gp
import predgrad_dense as pgd
import targets_dense as td
from append_context import grow_by_hand
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd.datagen import regression_data
from oracle import gp as ogp
from pred_tolerance import agg_tol, moment_tol, row_entries
from test_append_gpu import _check, _close, _compare_with_scratch, _contexts
from test_predcov_gpu import entry_tol, lib_noise

pytestmark = pytest.mark.gpu

RTOL = 1e-8     # tests/test_gpu_parity.py
C_SEVEN = [150, 40, 1, 130, 17, 40, 0]
TB = at.TB


def _routes(T):
    c = C_SEVEN if T.L == 7 else [20] * T.L
    Xt = np.asfortranarray(np.random.default_rng(5).uniform(size=(max(c), T.D)))
    return Xt, np.concatenate([[0], np.cumsum(c)]).astype(np.int64), np.concatenate([np.arange(k) for k in c]).astype(np.int64), c


def _append_keep(ctx, T):
    ptr, idx = T.add_csr()
    return ctx.append_rows(T.Xn, T.yn, ptr, idx, T.mean_new, keep_test=True)


def _keep(T, info_old=None):
    """Leading block columns of K_tn L^-T every leaf keeps: the kept blocks of the factor it reads (a COPY leaf: its source's)."""
    kb = T.kept_blocks(info_old)
    return [kb[T.src[l]] if T.op[l] == at.SHARE_COPY else kb[l] for l in range(T.L)]


def _expected_stats(T, c, keep):
    nb = [-(-len(o) // TB) for o in T.grown()[2]]
    routed = [l for l in range(T.L) if c[l] > 0]
    return dict(leaves_kept=sum(1 for l in routed if keep[l] > 0), block_columns_kept=sum(keep[l] for l in routed),
                block_columns_swept=sum(nb[l] - keep[l] for l in routed), leaves_from_block_0=sum(1 for l in routed if keep[l] == 0))


def _download_all(ctx, c, sizes):
    return [ctx.download_vt(l, c[l], sizes[l]) if c[l] else None for l in range(len(c))]


def _followers(ctx, T, c):
    """What reads K_tn L^-T and the moments after predict_run: covariance of the 150-, 130- and 1-row leaves (seven_leaves) or of
    leaves 0 and 39, input gradients, target means, the PoE aggregate."""
    Xg, yg, lists, _, _, mean = T.grown()
    cov = {l: ctx.predict_cov(l, c[l], with_noise=False) for l in ((0, 3, 2) if T.L == 7 else (0, 39))}
    dmu, dvar = ctx.predict_gradients()
    Y = np.stack([yg, np.cos(5.0 * Xg[:, 0])], axis=1)
    ctx.solve_targets(Y, np.stack([mean, np.zeros(T.L)], axis=1))
    return dict(cov=cov, dmu=dmu, dvar=dvar, tmu=ctx.predict_targets(), agg=ctx.aggregate(hipabi.AGG_POE, np.ones(T.L)), Y=Y)


def _sequence(tag, T, opts=(), run_before=True):
    """Contexts a and b through the sequences of the module docstring; the factor side is asserted here (it needs both contexts),
    everything else comes back as arrays."""
    Xt, rptr, ridx, c = _routes(T)
    n_old, n_new = [len(o) for o in T.lists], [len(o) for o in T.grown()[2]]
    a, b = _contexts(2)
    try:
        _, info_old, _ = at.fit_old(a, T, opts)
        a.set_test(Xt, rptr, ridx)
        V0 = None
        if run_before:
            a.predict_run()
            V0 = _download_all(a, c, n_old)
        routes0 = a.routes()
        mll_a, info_a, _ = _append_keep(a, T)
        st0 = a.resume_stats()
        assert a.route_total == int(rptr[-1]) and a.n_t == Xt.shape[0]       # the mirror of the resident set stays
        a.predict_run()
        out = dict(c=c, Xt=Xt, rptr=rptr, ridx=ridx, info_old=info_old, V0=V0, routes0=routes0, routes1=a.routes(), st0=st0,
                   st1=a.resume_stats(), append_stats=a.append_stats(), a=a.predict_fetch(), Va=_download_all(a, c, n_new))
        out["fa"] = _followers(a, T, c)
        a.predict_run()
        out["a_again"] = a.predict_fetch()
        mll_b, info_b, _ = at.fit_grown(b, T, opts)
        _compare_with_scratch(tag, a, b, T, mll_a, info_a, mll_b, info_b)
        b.set_test(Xt, rptr, ridx)
        b.predict_run()
        out.update(b=b.predict_fetch(), Vb=_download_all(b, c, n_new), fb=_followers(b, T, c))
        return out
    finally:
        _close(a, b)


CASES = {
    "seven iso relocate": lambda: (at.seven_leaves("iso", "relocate"), ()),
    "seven iso in_place": lambda: (at.seven_leaves("iso", "in_place"), ()),
    "seven iso split": lambda: (at.seven_leaves("iso", "split"), ()),
    "seven ard relocate": lambda: (at.seven_leaves("ard", "relocate"), ()),
    "small in_place": lambda: (at.many_small_leaves("in_place"), ()),
    "small relocate": lambda: (at.many_small_leaves("relocate"), ()),
    "seven iso relocate lanes=2": lambda: (at.seven_leaves("iso", "relocate"), ((hipabi.OPT_LANES, 2),)),
}
_DONE = {}


def _case(name):
    """Every case runs once; the tests below share what it left."""
    if name not in _DONE:
        T, opts = CASES[name]()
        _DONE[name] = (T, _sequence(name, T, opts))
    return _DONE[name]


def _dense_moments(T, l, xt):
    Xg, yg, lists, _, _, mean = T.grown()
    o = lists[l]
    if T.kind_id <= 2:
        g = ogp.GaussianProcess(Xg[o], yg[o], mean[l], ogp.make_kernel(T.kind_id, T.hyp[:-1]), T.hyp[-1], True).update_cholesky()
    else:
        g = dense_gp.DenseGP(T.kind_id, T.hyp, Xg[o], yg[o], mean[l])
    return g.prediction(xt)


# ------------------------------------------------------------------------------------------------ 1. same answers

@pytest.mark.parametrize("name", list(CASES))
def test_resumed_sweep_gives_the_answers_of_a_sweep_from_scratch(name):
    T, r = _case(name)
    Xg, yg, lists, _, _, _ = T.grown()
    c, rptr, ridx, Xt = r["c"], r["rptr"], r["ridx"], r["Xt"]
    noise = lib_noise(T.hyp[-1])
    yscale = max(1.0, float(np.max(np.abs(yg))))
    (ma, va), (mb, vb) = r["a"], r["b"]
    kss = np.ones(ma.size) * float(np.exp(2.0 * T.hyp[-2]))         # IsoSE / ArdMatern52: sigma^2
    tm, tv = moment_tol(mb, vb, kss, noise, yscale)
    _check(f"{name} mu a / b", ma, mb, tm)
    _check(f"{name} var a / b", va, vb, tv)
    for l in range(T.L):
        if c[l] == 0:
            continue
        s = slice(int(rptr[l]), int(rptr[l + 1]))
        mo, vo = _dense_moments(T, l, Xt[:c[l]])
        print(f"\n{name} leaf {l} against the dense leaf: max|dmu| {np.max(np.abs(ma[s] - mo)):.3g}  max|dvar| {np.max(np.abs(va[s] - vo)):.3g}")
        assert np.allclose(ma[s], mo, rtol=RTOL, atol=1e-9) and np.allclose(va[s], vo, rtol=RTOL, atol=1e-10), (name, l)
    fa, fb = r["fa"], r["fb"]
    for l, Sb in fb["cov"].items():
        _check(f"{name} predict_cov leaf {l}", fa["cov"][l], Sb, entry_tol(Sb, kss[:c[l]], noise))
    for l in range(T.L):
        if c[l] == 0:
            continue
        s = slice(int(rptr[l]), int(rptr[l + 1]))
        tdm, tdv = pgd.tolerances(T.kind_id, T.hyp[:-1], T.hyp[-1], np.asfortranarray(Xg[lists[l]]), yg[lists[l]],
                                  np.asfortranarray(Xt[:c[l]]), fb["dmu"][s], fb["dvar"][s])
        _check(f"{name} dmu leaf {l}", fa["dmu"][s], fb["dmu"][s], 2.0 * tdm)
        _check(f"{name} dvar leaf {l}", fa["dvar"][s], fb["dvar"][s], 2.0 * tdv)
    _check(f"{name} predict_targets", fa["tmu"], fb["tmu"], td.mu_tol(fb["tmu"], fb["Y"]))
    ent = row_entries(rptr, ridx, Xt.shape[0])
    am, av = agg_tol(hipabi.AGG_POE, mb, vb, tm, tv, ent, coef=np.ones(T.L))
    _check(f"{name} PoE mu", fa["agg"][0], fb["agg"][0], am)
    _check(f"{name} PoE var", fa["agg"][1], fb["agg"][1], av)
    # a repeated predict_run leaves the same bits
    assert np.array_equal(r["a_again"][0], ma) and np.array_equal(r["a_again"][1], va)


# ------------------------------------------------------------------------------------------------ 2. kept bits, what ran

@pytest.mark.parametrize("name", list(CASES))
def test_kept_columns_are_the_same_bits_and_the_stats_say_what_ran(name):
    """(max|V_a - V_b| / max|V_b| over the swept columns is printed, not asserted: the project has no tolerance for K_tn L^-T
    itself, the moment-level checks above are the assertion.  Largest value seen on an MI355X: DESIGN.md.)"""
    T, r = _case(name)
    c = r["c"]
    assert np.all(r["info_old"] == 0)
    keep = _keep(T, r["info_old"])
    worst = 0.0
    for l in range(T.L):
        if c[l] == 0:
            assert r["Va"][l] is None
            continue
        k = min(keep[l] * TB, len(T.lists[l]))
        assert np.array_equal(r["V0"][l][:, :k], r["Va"][l][:, :k]), (name, l)
        if k < r["Va"][l].shape[1]:
            d = float(np.max(np.abs(r["Va"][l][:, k:] - r["Vb"][l][:, k:])) / np.max(np.abs(r["Vb"][l][:, k:])))
            worst = max(worst, d)
            print(f"\n{name} leaf {l}: keep {keep[l]}, swept columns max|V_a - V_b| / max|V_b| {d:.3g}")
    print(f"\n{name}: largest swept-column difference {worst:.3g}")
    for x, y in zip(r["routes0"], r["routes1"]):
        assert np.array_equal(x, y)
    want = _expected_stats(T, c, keep)
    st0, st1 = r["st0"], r["st1"]
    print(f"\n{name}: {st1}")
    assert st0["block_columns_swept"] == -1 and st0["test_set_dropped"] == st1["test_set_dropped"] == 0
    for k, v in want.items():
        assert st1[k] == v, (name, k, st1[k], v)
        if k != "block_columns_swept":
            assert st0[k] == v
    assert (st1["bytes_relocated"] == 0) == ("in_place" in name), st1
    assert st1["bytes_relocated"] == st0["bytes_relocated"]
    assert (r["append_stats"]["bytes_relocated"] == 0) == ("in_place" in name)
    if "in_place" not in name:      # every kept 128 x 128 tile of every routed leaf moved once
        tiles = sum(keep[l] * -(-c[l] // TB) for l in range(T.L) if c[l] > 0)
        assert st1["bytes_relocated"] == tiles * TB * TB * 8


# ------------------------------------------------------------------------------------------------ 3. state

def _grown_fresh(ctx, T, Xt, rptr, ridx, opts=()):
    """A fresh context: the grown table, the test set, THEN the fit (standalone: dsmgp_set_joint(0)) and predict_run."""
    for o, v in opts:
        ctx.set_option(o, v)
    ctx.set_joint(False)
    Xg, yg, lists, op, src, mean = T.grown()
    ctx.set_train(Xg, yg)
    ctx.set_leaves(*at._csr(lists), T.kid, mean)
    ctx.set_hyper(0, T.kind_id, T.hyp)
    ctx.set_sharing(op, src, [0] * T.L)
    ctx.set_test(Xt, rptr, ridx)
    ctx.fit()
    ctx.predict_run()
    return ctx.predict_fetch()


def test_a_later_fit_sweeps_from_block_0_as_after_a_fresh_set_test():
    T = at.seven_leaves("iso", "relocate")
    Xt, rptr, ridx, c = _routes(T)
    a, b = _contexts(2)
    try:
        a.set_joint(False)
        at.fit_old(a, T)
        a.set_test(Xt, rptr, ridx)
        a.predict_run()
        _append_keep(a, T)
        a.predict_run()
        a.fit()
        a.predict_run()
        got = a.predict_fetch()
        ref = _grown_fresh(b, T, Xt, rptr, ridx)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        # ... and so does a fit that follows the call at once: the kept columns are not used
        _close(b)
        b = hipabi.Context(0)
        b.set_joint(False)
        at.fit_old(b, T)
        b.set_test(Xt, rptr, ridx)
        b.predict_run()
        _append_keep(b, T)
        b.fit()
        b.predict_run()
        got2 = b.predict_fetch()
        assert np.array_equal(got2[0], ref[0]) and np.array_equal(got2[1], ref[1])
        assert b.resume_stats()["block_columns_swept"] == -1
    finally:
        _close(a, b)


def test_a_test_set_without_a_sweep_is_kept_and_swept_in_full():
    T = at.seven_leaves("iso", "relocate")
    r = _sequence("no predict_run before", T, run_before=False)
    _, rb = _case("seven iso relocate")
    st = r["st1"]
    routed = sum(1 for k in r["c"] if k > 0)
    assert st["leaves_kept"] == 0 and st["block_columns_kept"] == 0 and st["bytes_relocated"] == 0 and st["test_set_dropped"] == 0
    assert st["leaves_from_block_0"] == routed
    assert st["block_columns_swept"] == sum(-(-len(o) // TB) for o, k in zip(T.grown()[2], r["c"]) if k > 0)
    # a full sweep on the grown plan (over the continued factors): results as in test 1
    mb, vb = rb["b"]
    tm, tv = moment_tol(mb, vb, np.ones(mb.size), lib_noise(T.hyp[-1]), max(1.0, float(np.max(np.abs(T.grown()[1])))))
    _check("no sweep before: mu", r["a"][0], mb, tm)
    _check("no sweep before: var", r["a"][1], vb, tv)


def test_without_a_test_set_the_call_is_append_rows_and_plain_append_rows_still_drops_the_set():
    T = at.seven_leaves("iso", "relocate")
    Xt, rptr, ridx, c = _routes(T)
    a, b, d = _contexts(3)
    try:
        with pytest.raises(hipabi.DsmgpError) as e:
            a.resume_stats()
        assert e.value.code == hipabi.E_STATE                      # before any call
        at.fit_old(a, T)
        at.fit_old(b, T)
        with pytest.raises(hipabi.DsmgpError) as e:
            a.download_vt(0, 1, 1)
        assert e.value.code == hipabi.E_STATE                      # no predict_run on the current fit
        mll_a, info_a, _ = _append_keep(a, T)
        mll_b, info_b, _ = at.append(b, T)
        assert np.array_equal(mll_a, mll_b) and np.array_equal(info_a, info_b) and a.append_stats() == b.append_stats()
        assert a.route_total == 0 and a.n_t == 0
        st = a.resume_stats()
        assert st == dict(leaves_kept=0, block_columns_kept=0, bytes_relocated=0, block_columns_swept=-1, leaves_from_block_0=0,
                          test_set_dropped=0)
        with pytest.raises(hipabi.DsmgpError) as e:
            a.predict_run()
        assert e.value.code == hipabi.E_STATE
        # plain append_rows with a resident, swept test set: the set goes, as tests/test_append_gpu.py asserts
        at.fit_old(d, T)
        d.set_test(Xt, rptr, ridx)
        d.predict_run()
        at.append(d, T)
        assert d.route_total == 0
        with pytest.raises(hipabi.DsmgpError) as e:
            d.predict_run()
        assert e.value.code == hipabi.E_STATE
        with pytest.raises(hipabi.DsmgpError) as e:
            d.routes()
        assert e.value.code == hipabi.E_STATE
        # download_vt: arguments
        a.set_test(Xt, rptr, ridx)
        a.predict_run()
        for leaf in (-1, T.L):
            with pytest.raises(hipabi.DsmgpError) as e:
                a.download_vt(leaf, 1, 1)
            assert e.value.code == hipabi.E_ARG
        V = np.empty((149, 320), order="F")
        assert a.lib.dsmgp_download_vt(a.h, 0, V.ctypes.data_as(hipabi._dp), 149) == hipabi.E_ARG      # ld < nt
        assert a.lib.dsmgp_download_vt(a.h, 6, None, 0) == 0                                             # no routed rows
        assert a.download_vt(0, 150, 320).shape == (150, 320)
    finally:
        _close(a, b, d)


def test_two_calls_before_the_sweep_keep_the_minimum():
    T = at.seven_leaves("iso", "relocate")
    Xt, rptr, ridx, c = _routes(T)
    adds1 = [x[:len(x) // 2] for x in T.adds]
    adds2 = [x[len(x) // 2:] for x in T.adds]
    T1 = at.Table("iso", T.X, T.y, T.lists, T.op, T.src, T.plen, T.mean, T.Xn, T.yn, adds1, None)
    Xg1, yg1, lists1, op1, src1, mean1 = T1.grown()
    T2 = at.Table("iso", Xg1, yg1, lists1, op1, src1, [0] * T.L, mean1, T.Xn, T.yn, adds2, T.mean_new)
    a = hipabi.Context(0)
    try:
        at.fit_old(a, T1)
        a.set_test(Xt, rptr, ridx)
        a.predict_run()
        _append_keep(a, T1)
        first = a.resume_stats()
        _append_keep(a, T2)
        second = a.resume_stats()
        a.predict_run()
        ma, va = a.predict_fetch()
        st = a.resume_stats()
    finally:
        a.close()
    # a leaf's kept count is the minimum of what it had (the first call's) and what the second call keeps of its factor
    k1, k2 = _keep(T1), _keep(T2)
    keep = [min(x, y) for x, y in zip(k1, k2)]
    routed = [l for l in range(T.L) if c[l] > 0]
    print(f"\ntwo calls: {first} then {st}")
    assert first["block_columns_kept"] == sum(k1[l] for l in routed)
    assert second["block_columns_kept"] == st["block_columns_kept"] == sum(keep[l] for l in routed)
    nb = [-(-len(o) // TB) for o in T2.grown()[2]]
    assert st["block_columns_swept"] == sum(nb[l] - keep[l] for l in routed)
    # the leaves hold the rows of T.grown() in its order (as values): context b of the shared case is the reference
    _, rb = _case("seven iso relocate")
    mb, vb = rb["b"]
    yscale = max(1.0, float(np.max(np.abs(T.grown()[1]))))
    tm, tv = moment_tol(mb, vb, np.ones(mb.size), lib_noise(T.hyp[-1]), yscale)
    _check("two calls mu", ma, mb, tm)
    _check("two calls var", va, vb, tv)


def test_failed_owner_sweeps_from_block_0_and_gets_nan():
    X, y, Xn, yn, lists, adds, kid, mean = at.failed_owner_table()
    L = len(lists)
    Xt = np.asfortranarray(np.random.default_rng(8).uniform(size=(20, X.shape[1])))
    rptr, ridx = np.arange(L + 1) * 20, np.tile(np.arange(20), L)
    a, b = _contexts(2)
    try:
        a.set_train(X, y)
        a.set_leaves(*at._csr(lists), kid, mean)
        grown = [np.concatenate([o, X.shape[0] + x]) for o, x in zip(lists, adds)]
        b.set_train(np.vstack([X, Xn]), np.concatenate([y, yn]))
        b.set_leaves(*at._csr(grown), kid, mean)
        for ctx in (a, b):
            for k, (kind, hyp) in at.FAILED_HYP.items():
                ctx.set_hyper(k, kind, hyp)
        _, info_old, _ = a.fit()
        assert info_old[0] == 4 and np.all(info_old[1:] == 0)
        a.set_test(Xt, rptr, ridx)
        a.predict_run()
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in adds])])
        _, info, _ = a.append_rows(Xn, yn, ptr, np.concatenate(adds), keep_test=True)
        a.predict_run()
        st = a.resume_stats()
        print(f"\nfailed owner: {st}")
        assert info[0] == 4 and st["leaves_from_block_0"] == 1 and st["leaves_kept"] == 3
        ma, va = a.predict_fetch()
        b.fit()
        b.set_test(Xt, rptr, ridx)
        b.predict_run()
        mb, vb = b.predict_fetch()
        assert np.all(np.isnan(ma[:20])) and np.all(np.isnan(va[:20])) and np.all(np.isnan(mb[:20]))
        noise = lib_noise(at.FAILED_HYP[0][1][-1])
        tm, tv = moment_tol(mb[20:], vb[20:], np.ones(mb.size - 20) * float(np.exp(2.0 * at.FAILED_HYP[0][1][-2])), noise,
                            max(1.0, float(np.max(np.abs(y)))))
        _check("failed owner: the others, mu", ma[20:], mb[20:], tm)
        _check("failed owner: the others, var", va[20:], vb[20:], tv)
    finally:
        _close(a, b)


# ------------------------------------------------------------------------------------------------ 4. determinism

def test_two_runs_of_the_sequence_agree_bitwise():
    T, r = _case("seven iso relocate")
    r2 = _sequence("second run", T)
    assert np.array_equal(r["a"][0], r2["a"][0]) and np.array_equal(r["a"][1], r2["a"][1])
    for V, W in zip(r["Va"], r2["Va"]):
        assert (V is None and W is None) or np.array_equal(V, W)
    assert r["st1"] == r2["st1"]


# ------------------------------------------------------------------------------------------------ 5. add_data on the device

@pytest.mark.parametrize("family", ["dsmgp", "poe", "gp"])
def test_add_data_keeps_the_candidates_resident(family):
    N, D = 3000, 3
    X, y, Xt = regression_data(N, D, n_test=200, seed=900)
    Xn, yn, _ = regression_data(40, D, n_test=1, seed=901)
    kw = dict(kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1))

    def build():
        if family == "dsmgp":
            return dsm.buildDSMGP(X, y, 3, 4, M=60, seed=4, **kw)
        if family == "poe":
            return dsm.buildPoE(X, y, 6, meanFun=None, seed=4, **kw)
        g = dsm.GaussianProcess(X[:700], y[:700], **kw)
        dsm.fit(g)
        return g

    pred = (lambda m_: dsm.prediction(m_, Xt)) if family == "gp" else (lambda m_: dsm.predict(m_, Xt))
    m, h = build(), build()
    tm, th = (m.model, h.model) if family == "gp" else (m, h)
    try:
        pred(m)                                                         # the candidates become resident, K_tn L^-T is swept
        cache = tm._route_cache
        assert cache is not None and cache["uploaded"]
        sec = dsm.add_data(m, Xn, yn, keep_test=True)
        assert sec.fallback is False and sec.resume_stats is not None and sec.resume_stats["test_set_dropped"] == 0
        assert tm._route_cache is cache and cache["uploaded"]
        assert dsm.add_data.__defaults__[-1] is False
        if family != "gp":
            dsm.update(m)
        mu, var = pred(m)
        st = tm.ctx.resume_stats()
        print(f"\nadd_data keep_test {family}: {st}")
        assert st["block_columns_kept"] > 0 and st["block_columns_swept"] >= 0
        grow_by_hand(family, h, Xn, yn)
        if family != "gp":
            dsm.update(h)
        mo, vo = pred(h)
        assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9) and np.allclose(var, vo, rtol=RTOL, atol=1e-9)     # test_append_gpu's
    finally:
        tm.ctx.close()
        th.ctx.close()
