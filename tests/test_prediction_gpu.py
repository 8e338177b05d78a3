"""GPU suite: prediction, aggregation and scores against 50-digit references (tests/golden/gp_pred.npz, written by
tests/golden/make_pred_golden.py).

The prediction of a leaf is a sweep of its test rows through the factor: K_tn tiles (fused into the update tasks for
D <= 32, from the Gram launch above), update and panel-solve launches whose epilogues accumulate macc / sacc, split-K
reduces, and pred_finish_kernel -- or, with the rows riding through the factorisation (joint), the same epilogues inside
fit, and pred_mu_kernel + pred_var_kernel for COPY / PREFIX leaves.  The cases reach the row- and test-tile edges (128),
the standalone sweep's split-K and fused steps, two leaf lanes, every kernel kind (ArdLinear with unequal l_d), and the
aggregation and score kernels on a table whose rBCM groups miss rows and whose offset targets make the mixture variance
cancel.  Every tolerance comes from tests/pred_tolerance.py."""
import functools
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi
from pred_tolerance import EPS, agg_tol, alpha_tol, mll_tol, moment_tol, row_entries, score_tol

pytestmark = pytest.mark.gpu

OFFSET = 1000.0       # make_pred_golden.OFFSET
FAMILIES = {"mixture": (hipabi.AGG_MIXTURE, False), "mixture_plain": (hipabi.AGG_MIXTURE, True), "poe": (hipabi.AGG_POE, False),
            "gpoe": (hipabi.AGG_GPOE, False), "rbcm": (hipabi.AGG_RBCM, False)}


def _load():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_pred.npz"))
    single, table, config1 = {}, {}, {}
    for key in z.files:
        head, rest = key.split("/", 1)
        if head == "single":
            name, field = rest.split("/")
            single.setdefault(name, {})[field] = z[key]
        elif head == "table":
            table[rest] = z[key]
        else:
            config1[rest] = z[key]
    return single, table, config1


SINGLE, TABLE, CONFIG1 = _load()


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _check(tag, got, ref, tol):
    """Every element within its tolerance; prints the worst error and error / tolerance."""
    got, ref, tol = (np.asarray(a, dtype=np.float64) for a in (got, ref, tol))
    err = np.abs(got - ref)
    ratio = err / tol
    worst = int(np.argmax(ratio)) if ratio.size else 0
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    assert np.all(err <= tol), (tag, worst, got.flat[worst], ref.flat[worst], tol.flat[worst])


# ------------------------------------------------------------------------------------- (a) single leaves

_SINGLE_PARAMS = [(name, path, fg) for name in sorted(SINGLE) for path in ("standalone", "joint") for fg in (1, 0)
                  if fg == 1 or SINGLE[name]["X"].shape[1] <= 32]          # above D = 32 OPT_FUSED_GRAM has no effect


@pytest.mark.parametrize("name,path,fused_gram", _SINGLE_PARAMS)
def test_single_leaf_prediction_against_50_digit_references(ctx, name, path, fused_gram):
    """One leaf, predicted by the standalone sweep (test rows registered after fit) or jointly (registered before: the
    rows ride through fit and predict only finishes), with the Gram values fused into the update tasks or read from the
    Gram launch.  mu and sigma^2 of every row, alpha and the mll within their tolerances; the row listed twice gives the
    same bits; the far rows give mu = mean and sigma^2 = k** + noise to eps."""
    c = SINGLE[name]
    X, y, Xt = c["X"], c["y"], c["Xt"]
    kind, mean = int(c["kind"]), float(c["mean"])
    hyp = np.concatenate([c["loghyp"], [float(c["logNoise"])]])
    noise = np.exp(2.0 * float(c["logNoise"]))
    n, nt = X.shape[0], Xt.shape[0]
    ctx.set_option(hipabi.OPT_FUSED_GRAM, fused_gram)
    ctx.set_profile(2)
    try:
        ctx.set_train(X, y)
        ctx.set_leaves([0, n], np.arange(n), [0], [mean])
        ctx.set_hyper(0, kind, hyp)
        if path == "joint":
            ctx.set_test(Xt, [0, nt], np.arange(nt))
            mll, info, _ = ctx.fit()
            ctx.predict_run()
            mu, var = ctx.predict_fetch()
        else:
            mll, info, _ = ctx.fit()
            mu, var = ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
        t = ctx.timings()
        _, alpha = ctx.download_factor(0, n, factor=False)
    finally:
        ctx.set_profile(0)
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)
    assert info[0] == 0
    if path == "joint":           # the rows rode through fit: no sweep of predict's own
        assert t["predict_update"] == 0.0 and t["predict_trsm"] == 0.0
    tag = f"{name} {path} fused_gram={fused_gram}"
    _check(tag + " mll", mll[0], c["mll"], mll_tol(c["mll"], c["cond"]))
    _check(tag + " alpha", alpha, c["alpha"], alpha_tol(c["alpha"], c["cond"]))
    tmu, tvar = moment_tol(c["mu"], c["var"], c["kss"], noise, max(1.0, float(np.max(np.abs(y)))))
    _check(tag + " mu", mu, c["mu"], tmu)
    _check(tag + " var", var, c["var"], tvar)
    d0, d1 = (int(i) for i in c["dup"])
    assert mu[d0].tobytes() == mu[d1].tobytes() and var[d0].tobytes() == var[d1].tobytes(), (mu[[d0, d1]], var[[d0, d1]])
    for p in c["far"]:
        s = float(c["kss"][p]) + noise
        assert abs(mu[p] - mean) <= EPS * abs(mean) and abs(var[p] - s) <= 4 * EPS * s, (p, mu[p], mean, var[p], s)


# ------------------------------------------------------------------------------------- (b) the leaf table

def _table_entry_tol(offset):
    T = TABLE
    kinds, hyp, hl = T["kinds"], T["hyp"], T["hyp_len"]
    noise_k = np.array([np.exp(2.0 * hyp[k][hl[k] - 1]) for k in range(len(kinds))])
    ent_leaf = np.repeat(np.arange(T["kid"].size), np.diff(T["route_ptr"]))
    noise = noise_k[T["kid"][ent_leaf]]
    y = T["y"] + (OFFSET if offset else 0.0)
    return moment_tol(T["mu_off"] if offset else T["mu"], T["var"], T["kss"], noise, max(1.0, float(np.max(np.abs(y)))))


@functools.lru_cache(maxsize=None)
def _table_tolerances():
    """Per-entry tolerances of both target variants, and per family the aggregate's and the scores' tolerances."""
    T = TABLE
    nt = T["Xt"].shape[0]
    ent = row_entries(T["route_ptr"], T["route_idx"], nt)
    D = T["Xt"].shape[1]
    pk = int(T["prior_kid"])
    kss_prior = (T["Xt"] ** 2) @ np.exp(-2.0 * T["hyp"][pk][:D])          # the prior kernel is ArdLinear
    noise_prior = float(np.exp(2.0 * T["hyp"][pk][T["hyp_len"][pk] - 1]))
    out = {"entry": _table_entry_tol(False), "entry_off": _table_entry_tol(True)}
    for fam_name, (fam, plain) in list(FAMILIES.items()) + [("mixture_off", (hipabi.AGG_MIXTURE, False))]:
        off = fam_name == "mixture_off"
        coef = {"poe": np.ones(T["kid"].size), "gpoe": T["beta"]}.get(fam_name, T["w_mix"])
        tm_e, tv_e = out["entry_off" if off else "entry"]
        tm, tv = agg_tol(fam, T["mu_off" if off else "mu"], T["var"], tm_e, tv_e, ent, S1=T.get(f"agg/{fam_name}/S1"),
                         coef=coef, group=T["group"], G=int(T["G"]), plain=plain, kss_prior=kss_prior, noise_prior=noise_prior)
        yt = T["yt"] + (OFFSET if off else 0.0)
        ts = score_tol(yt, T[f"agg/{fam_name}/mu"], T[f"agg/{fam_name}/var"], tm, tv)
        out[fam_name] = (tm, tv, ts)
    return out


def _table_setup(ctx, offset):
    T = TABLE
    ctx.set_train(T["X"], T["y"] + (OFFSET if offset else 0.0))
    ctx.set_leaves(T["obs_ptr"], T["obs_idx"], T["kid"], T["mean_off"] if offset else T["mean"])
    ctx.set_sharing(T["op"], T["src"], T["plen"])
    for k in range(T["kinds"].size):
        ctx.set_hyper(k, int(T["kinds"][k]), T["hyp"][k][:T["hyp_len"][k]])


def _agg_args(fam_name):
    T = TABLE
    if fam_name == "rbcm":
        return dict(leaf_group=T["group"], n_groups=int(T["G"]))
    return dict(leaf_coef={"poe": np.ones(T["kid"].size), "gpoe": T["beta"]}.get(fam_name, T["w_mix"]))


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("fused_steps", [1, 0])
@pytest.mark.parametrize("path", ["joint", "standalone"])
def test_leaf_table_prediction_aggregation_and_scores(ctx, path, fused_steps, lanes):
    """41 leaves through the low-level ABI: 8 observation sets (n = 130 .. 512) over 5 replicas -- >= 32 leaves in the
    shallow block steps, so with DSMGP_OPT_FUSED_STEPS = 1 they run fused (tile_fused8_kernel, and in the standalone sweep
    psweep.f8) -- a declared COPY and a PREFIX leaf (joint: the pred_mu / pred_var slow path), one leaf without routed rows,
    10 .. 150 routed rows per leaf (second test tile), four kernel ids (IsoSE, ArdSE, IsoLinear, ArdLinear), one or two
    leaf lanes.  Per entry mu / sigma^2 and per leaf the mll against the fixture; every family through dsmgp_aggregate and
    through aggregate_partial + aggregate_finish, and the scores; then the targets offset by 1000 for the mixture."""
    T = TABLE
    tols = _table_tolerances()
    nt = T["Xt"].shape[0]
    tag = f"table {path} fused_steps={fused_steps} lanes={lanes}"
    ctx.set_option(hipabi.OPT_FUSED_STEPS, fused_steps)
    ctx.set_option(hipabi.OPT_LANES, lanes)
    try:
        for offset in (False, True):
            _table_setup(ctx, offset)
            if path == "joint":
                ctx.set_test(T["Xt"], T["route_ptr"], T["route_idx"])
                mll, info, _ = ctx.fit()
                fused = ctx.work_fused()[1]
                ctx.predict_run()
                mu, var = ctx.predict_fetch()
            else:
                mll, info, _ = ctx.fit()
                fused = ctx.work_fused()[1]
                mu, var = ctx.predict_leaves(T["Xt"], T["route_ptr"], T["route_idx"])
            assert np.all(info == 0)
            assert (fused > 0) if fused_steps else (fused == 0), fused
            assert ctx.lanes() == lanes
            otag = tag + (" offset" if offset else "")
            mref = T["mll_off"] if offset else T["mll"]
            _check(otag + " mll", mll, mref, mll_tol(mref, T["cond"]))
            tmu, tvar = tols["entry_off" if offset else "entry"]
            _check(otag + " mu", mu, T["mu_off"] if offset else T["mu"], tmu)
            _check(otag + " var", var, T["var"], tvar)
            for fam_name in (["mixture_off"] if offset else list(FAMILIES)):
                fam, plain = FAMILIES.get(fam_name, (hipabi.AGG_MIXTURE, False))
                tm, tv, ts = tols[fam_name]
                prior = int(T["prior_kid"]) if fam == hipabi.AGG_RBCM else 0
                rm, rv = T[f"agg/{fam_name}/mu"], T[f"agg/{fam_name}/var"]
                part = ctx.aggregate_partial(fam, **_agg_args(fam_name))
                m2, v2 = ctx.aggregate_finish(part, plain=plain, prior_kernel_id=prior)
                _check(f"{otag} {fam_name} partial+finish mu", m2, rm, tm)
                _check(f"{otag} {fam_name} partial+finish var", v2, rv, tv)
                m1, v1 = ctx.aggregate(fam, plain=plain, prior_kernel_id=prior, **_agg_args(fam_name))
                _check(f"{otag} {fam_name} mu", m1, rm, tm)
                _check(f"{otag} {fam_name} var", v1, rv, tv)
                sc = ctx.scores(T["yt"] + (OFFSET if offset else 0.0))
                _check(f"{otag} {fam_name} scores", [sc[k] for k in hipabi.SCORE_NAMES], T[f"agg/{fam_name}/scores"], ts)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_LANES, 0)


# ------------------------------------------------------------------------------------- (c) config 1 end to end

def test_config1_end_to_end_against_50_digit_references():
    """The README example (BASELINE config 1) through the Python API: buildDSMGP -> update -> predict -> scores.  Leaf mlls,
    the root mll of update!, the per-leaf moments in the model's routing, the mixture and the scores against the 50-digit
    values of the reference's literal log-domain recursion."""
    C = CONFIG1
    x, y, xt, yt = C["x"], C["y"], C["xt"], C["yt"]
    m = dsm.buildDSMGP(x.reshape(-1, 1), y, 3, 4, M=10, kernel=dsm.IsoSE(1.0, 1.0), meanFun=dsm.ConstMean(float(np.mean(x))),
                       seed=11)
    lt = mll_tol(C["leaf_mll"], C["cond"])
    _check("config1 leaf mll", m.leaf_mll, C["leaf_mll"], lt)
    z = dsm.update(m)
    # a split node adds its children's errors, a sum node's log-sum-exp moves by at most its largest child's: the root moves
    # by at most the sum over the leaves
    _check("config1 root mll", z, C["root_mll"], np.sum(lt) + 16 * EPS * abs(float(C["root_mll"])))
    mu, var = dsm.predict(m, xt)
    ptr, idx = m.ctx.routes()
    assert np.array_equal(ptr, C["route_ptr"])
    pos = {}                                   # (leaf, row) -> entry of the fixture; the device's entries in its own order
    for l in range(ptr.size - 1):
        assert sorted(idx[ptr[l]:ptr[l + 1]]) == sorted(C["route_idx"][ptr[l]:ptr[l + 1]])
        pos.update({(l, int(r)): e for e, r in enumerate(C["route_idx"][ptr[l]:ptr[l + 1]], start=int(ptr[l]))})
    perm = np.array([pos[(l, int(idx[e]))] for l in range(ptr.size - 1) for e in range(ptr[l], ptr[l + 1])], dtype=np.int64)
    lmu, lvar = m.ctx.predict_fetch()
    lmu[perm], lvar[perm] = lmu.copy(), lvar.copy()      # into the fixture's order
    tmu_e, tvar_e = moment_tol(C["leaf_mu"], C["leaf_var"], np.full(C["leaf_var"].size, np.exp(2.0)), np.exp(2.0),
                               max(1.0, float(np.max(np.abs(y)))))
    _check("config1 leaf mu", lmu, C["leaf_mu"], tmu_e)
    _check("config1 leaf var", lvar, C["leaf_var"], tvar_e)
    ent = row_entries(C["route_ptr"], C["route_idx"], xt.shape[0])
    tm, tv = agg_tol(hipabi.AGG_MIXTURE, C["leaf_mu"], C["leaf_var"], tmu_e, tvar_e, ent, S1=C["S1"], coef=C["leaf_w"])
    _check("config1 mu", mu, C["mu"], tm)
    _check("config1 var", var, C["var"], tv)
    sc = dsm.scores(m, yt)
    _check("config1 scores", [sc[k] for k in hipabi.SCORE_NAMES], C["scores"], score_tol(yt, C["mu"], C["var"], tm, tv))
