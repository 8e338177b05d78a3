"""What the tests of dsmgp_aggregate_gradients* share: the family specifications, the host oracle with its tolerance, and a small
leaf table whose test rows reach none, one and many leaves.

Oracle: dsm.aggregate_input_gradients (pinned to the 50-digit agg/* arrays of tests/golden/gp_predgrad.npz by
test_predgrad_host.py) on the SAME context's predict_fetch() and predict_gradients() and pred_tolerance.row_entries.
Tolerance: twice the one test_predgrad_host.py::test_aggregation_against_50_digits derives -- every input carries 4 eps of its
magnitude through predgrad_dense.aggregate_gradients over Prop, plus 64 eps of the result; doubled because both sides round."""
import math

import numpy as np

import deepstructuredmixtures_amd as dsm
import dense_kernels as dk
import predgrad_dense as pgd
from deepstructuredmixtures_amd import datagen
from pred_tolerance import ATOL, EPS, RTOL, Prop, agg_tol, aggregate, row_entries

MIXTURE, POE, GPOE, RBCM = 0, 1, 2, 3


def spec(family, coef=None, group=None, G=0, plain=False, prior_kid=0):
    return dict(family=family, coef=None if coef is None else np.asarray(coef, dtype=np.float64),
                group=None if group is None else np.asarray(group, dtype=np.int32), G=int(G), plain=bool(plain), prior_kid=int(prior_kid))


def device_moments(ctx, s, fetch=True):
    return ctx.aggregate(s["family"], s["coef"], s["group"], s["G"], plain=s["plain"], prior_kernel_id=s["prior_kid"], fetch=fetch)


def device_gradients(ctx, s, **kw):
    """aggregate + aggregate_gradients of one family on the context's current prediction."""
    device_moments(ctx, s, fetch=False)
    return ctx.aggregate_gradients(plain=s["plain"], prior_kernel_id=s["prior_kid"], **kw)


def prior_terms(s, Xt, prior):
    """The rBCM prior of `aggregate_input_gradients`: prior = (kind, loghyp without the noise, logNoise) of the prior kernel id."""
    if s["family"] != RBCM:
        return {}
    kind, loghyp, logNoise = prior
    return dict(kss_prior=dk.prior_diag(kind, loghyp, Xt), noise_prior=math.exp(2.0 * float(logNoise)), dkss_prior=dk.prior_dx(kind, loghyp, Xt))


def oracle(s, entries, Xt, route_ptr, route_idx, prior=None, entry_tol=None):
    """(dmu, dvar, tol dmu, tol dvar), each (n_t, D), from the per-entry arrays `entries` = (mu, var, dmu, dvar).  A row
    without entries has no per-entry input: its tolerance is the 64 eps of the result alone (the prior's own terms are the same
    float64 operations on both sides)."""
    mu, var, dmu, dvar = (np.asarray(a, dtype=np.float64) for a in entries)
    n_t, D = Xt.shape
    ent = row_entries(route_ptr, route_idx, n_t)
    kw = dict(coef=s["coef"], group=s["group"], G=s["G"], plain=s["plain"], **prior_terms(s, Xt, prior))
    with np.errstate(all="ignore"):
        gm, gv = dsm.aggregate_input_gradients(s["family"], mu, var, dmu, dvar, ent, **kw)
        P = lambda a: [Prop(v, 4 * EPS * abs(v)) for v in a]                            # noqa: E731
        PT = lambda a, t: [Prop(v, e) for v, e in zip(a, t)]                            # noqa: E731
        pkw = dict(kw)
        if s["family"] == RBCM:
            pkw.update(kss_prior=P(kw["kss_prior"]), dkss_prior=[P(r) for r in kw["dkss_prior"]])
        if entry_tol is None:       # the inputs are exact: the function's own rounding
            pin = (P(mu), P(var), [P(r) for r in dmu], [P(r) for r in dvar])
        else:                       # the inputs are another kernel's: (tol mu, tol var, tol dmu, tol dvar) per entry
            pin = (PT(mu, entry_tol[0]), PT(var, entry_tol[1]), [PT(r, t) for r, t in zip(dmu, entry_tol[2])],
                   [PT(r, t) for r, t in zip(dvar, entry_tol[3])])
        tm, tv = pgd.aggregate_gradients(s["family"], *pin, ent, log=Prop.log, **pkw)
    err = lambda rows: np.array([[float(Prop.of(v).e) for v in r] if r else [0.0] * D for r in rows]).reshape(n_t, D)     # noqa: E731
    return gm, gv, 2.0 * (err(tm) + 64 * EPS * np.abs(gm)), 2.0 * (err(tv) + 64 * EPS * np.abs(gv))


def moments_oracle(s, mu, var, Xt, route_ptr, route_idx, prior=None, tol_mu=None):
    """(mu, var, tol mu, tol var) per test row: pred_tolerance.aggregate in float64 on the per-entry moments, with agg_tol's
    tolerance doubled (both sides round) for per-entry tolerances of 4 eps of the magnitude (`tol_mu`: another one for the
    means).  Rows without entries are NaN here: the caller compares them with dsmgp_aggregate's rows."""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    n_t = Xt.shape[0]
    ent = row_entries(route_ptr, route_idx, n_t)
    rows = np.array([r for r in range(n_t) if ent[r]], dtype=np.int64)
    sub = [ent[r] for r in rows]
    kw = dict(coef=s["coef"], group=s["group"], G=s["G"], plain=s["plain"])
    if s["family"] == RBCM:
        p = prior_terms(s, Xt, prior)
        kw.update(kss_prior=list(p["kss_prior"][rows]), noise_prior=p["noise_prior"])
    out = [np.full(n_t, np.nan) for _ in range(4)]
    if rows.size:
        am, av = aggregate(s["family"], list(mu), list(var), sub, log=np.log, **kw)
        S1 = None
        if s["family"] == MIXTURE:
            S1 = [sum(float(s["coef"][l]) * mu[e] ** 2 for l, e in er) for er in sub]
        tm, tv = agg_tol(s["family"], mu, var, 4 * EPS * np.abs(mu) if tol_mu is None else tol_mu, 4 * EPS * np.abs(var), sub, S1=S1, **kw)
        for o, v in zip(out, (am, av, 2.0 * tm, 2.0 * tv)):
            o[rows] = np.asarray(v, dtype=np.float64)
    return out


def columns_oracle(ctx, s, Xt, route_ptr, route_idx, prior=None):
    """The host references of both column calls from the context's own per-entry arrays: (mu, var, tol mu, tol var), each
    (n_t, Q), and (dmu, dvar, tol dmu, tol dvar), each (n_t, D, Q)."""
    _, var_l = ctx.predict_fetch()
    tmu = ctx.predict_targets()
    tdm = ctx.predict_targets_gradients()
    _, dvar_l = ctx.predict_gradients()
    Q = tmu.shape[1]
    mom = [moments_oracle(s, tmu[:, q], var_l, Xt, route_ptr, route_idx, prior) for q in range(Q)]
    grd = [oracle(s, (tmu[:, q], var_l, tdm[:, :, q], dvar_l), Xt, route_ptr, route_idx, prior) for q in range(Q)]
    return tuple(np.stack([m[k] for m in mom], axis=1) for k in range(4)), tuple(np.stack([g[k] for g in grd], axis=2) for k in range(4))


def context_entries(ctx):
    return ctx.predict_fetch() + ctx.predict_gradients()


def check(tag, got, ref, tol, rows=None):
    """Every element of the rows within its tolerance (NaN and infinities must match as such); prints the worst err / tol."""
    got, ref, tol = (np.asarray(a, dtype=np.float64) for a in (got, ref, tol))
    if rows is not None:
        got, ref, tol = got[rows], ref[rows], tol[rows]
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (tag, "non-finite entries differ")
    err = np.abs(got[fin] - ref[fin])
    ratio = err / np.where(tol[fin] > 0, tol[fin], 1.0)
    ratio[(tol[fin] == 0) & (err == 0)] = 0.0
    worst = float(np.max(ratio)) if ratio.size else 0.0
    print(f"\n{tag}: {int(fin.sum())} finite values, max err {float(np.max(err)) if err.size else 0.0:.3g}, worst err/tol {worst:.3g}")
    assert np.all(err <= tol[fin]), (tag, worst)


# ---------------------------------------------------------------------------------------------- a small leaf table
N_LEAVES, KID_SE, KID_LIN = 6, 0, 1


def small_table(n_t, D, seed):
    """Six leaves of 30 .. 55 training rows over N = 260 rows, kernel ids 0 (IsoSE) and 1 (ArdLinear); n_t test rows of which
    row r reaches (r mod 4 == 0 and n_t > 2: no leaf; r mod 4 == 1: one leaf; else: three to six leaves).  With the groups
    leaf mod 3 some rows see two of the three groups only (the rows with one leaf see one).  Returns a dict."""
    N = 260
    X = datagen.uniform(seed, 0, N * D).reshape((N, D), order="F")
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * datagen.normal(seed + 1, 0, N) + 0.7
    Xt = np.asfortranarray(datagen.uniform(seed + 2, 0, n_t * D).reshape((n_t, D), order="F") * 1.1 - 0.05)
    rng = np.random.default_rng(seed)
    sizes = [30, 41, 55, 33, 48, 37]
    obs = [np.sort(rng.choice(N, size=n, replace=False)) for n in sizes]
    obs_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    reach = [[] for _ in range(N_LEAVES)]
    for r in range(n_t):
        if r % 4 == 0 and n_t > 2:
            continue
        if r % 4 == 1:
            leaves = [int(rng.integers(N_LEAVES))]
        elif r % 4 == 2:
            leaves = sorted(rng.choice(N_LEAVES, size=3, replace=False).tolist())
        else:
            leaves = list(range(N_LEAVES)) if r % 8 == 3 else [0, 3, 1, 4]      # [0, 3, 1, 4]: groups 0 and 1 only
        for l in leaves:
            reach[l].append(r)
    route_ptr = np.concatenate([[0], np.cumsum([len(v) for v in reach])]).astype(np.int64)
    route_idx = np.array([r for v in reach for r in v], dtype=np.int64)
    hyp_se = np.array([np.log(0.4 * np.sqrt(D)), 0.1, np.log(0.1)])
    hyp_lin = np.concatenate([np.log(np.linspace(0.8, 1.6, D) * np.sqrt(D)), [0.0], [np.log(0.15)]])
    kid = np.array([KID_SE, KID_LIN, KID_SE, KID_SE, KID_LIN, KID_SE], dtype=np.int32)
    mean = np.array([float(np.mean(y[o])) for o in obs])
    L = N_LEAVES
    w = np.linspace(1.0, 2.0, L)
    specs = dict(mixture=spec(MIXTURE, coef=w / w.sum()), plain=spec(MIXTURE, coef=w / w.sum(), plain=True), poe=spec(POE, coef=np.ones(L)),
                 gpoe=spec(GPOE, coef=np.full(L, 0.5)), rbcm=spec(RBCM, group=np.arange(L) % 3, G=3, prior_kid=KID_LIN))
    return dict(X=np.asfortranarray(X), y=y, Xt=Xt, obs_ptr=obs_ptr, obs_idx=np.concatenate(obs).astype(np.int64), kid=kid, mean=mean,
                route_ptr=route_ptr, route_idx=route_idx, hyp={KID_SE: (0, hyp_se), KID_LIN: (3, hyp_lin)}, specs=specs,
                prior=(3, hyp_lin[:-1], hyp_lin[-1]))


def small_setup(ctx, t):
    ctx.set_train(t["X"], t["y"])
    ctx.set_leaves(t["obs_ptr"], t["obs_idx"], t["kid"], t["mean"])
    for k, (kind, hyp) in t["hyp"].items():
        ctx.set_hyper(k, kind, hyp)


def small_predict(ctx, t):
    """Fit, register the rows, run the prediction; every leaf must factorise."""
    small_setup(ctx, t)
    _, info, _ = ctx.fit()
    assert np.all(info == 0)
    ctx.set_test(t["Xt"], t["route_ptr"], t["route_idx"])
    ctx.predict_run()
