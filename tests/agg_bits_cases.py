"""The cases whose raw float64 outputs tests/golden/agg_parent.npz records from the eight aggregation entry points
(dsmgp_aggregate*, dsmgp_aggregate_gradients*, dsmgp_aggregate_columns*) and dsmgp_scores: the smallest shapes at which a family
rule of csrc/kernels_agg.hpp, a row walk or a plane layout can go wrong.  Shared by the recorder
tests/golden/make_agg_parent.py and by tests/test_agg_bits_gpu.py, which asserts the recorded bits.  Inputs come from datagen's
counter streams, from fixed formulas and, for the observation sets, the routes and the failed-leaf rows, from NumPy's
default_rng (PCG64): the fixture is tied to those streams as agg_gradients_cases.small_table is.

    table/<n_t>x<D>     agg_gradients_cases.small_table: (1, 3); (40, 11): one full AGG_DC chunk of input dimensions and a partial
                        one; (257, 1): both sides of the 256-thread block.  Rows with no, one and up to six entries; rBCM rows that
                        see one, two or three of the G = 3 groups; the rBCM prior is the ArdLinear id (ds/dx != 0)
    clamp               the arrangement of test_agg_gradients_gpu.test_clamped_leaf_variance_is_a_constant (its own rows: the
                        table's inputs of size 1 give no leaf variance <= 0): mixture and plain
    failed_leaf         the arrangement of test_agg_gradients_gpu.test_failed_leaf_gives_nan_rows: NaN rows, every family

Every case runs each of its families with Q = 3 target columns made from y.  Per family: partial (aggregate_partial), mu / var
(aggregate), scores (the five of SCORE_NAMES), grad_partial (aggregate_gradients_partial), dmu / dvar (aggregate_gradients),
col_mu / col_var (aggregate_columns), col_dmu / col_dvar (aggregate_columns_gradients).  Test infrastructure only."""
import numpy as np

import agg_gradients_cases as ac
from deepstructuredmixtures_amd import hipabi

TABLES = ((1, 3), (40, 11), (257, 1))
Q = 3


def columns(X, y):
    """Q columns over the training rows: column 0 is y; the others rescale and shift it and add a smooth term of the first input."""
    j = np.arange(Q)
    return np.asfortranarray(y[:, None] * (1.0 + 0.3 * j)[None, :] + (0.2 * j)[None, :] * np.cos(5.0 * X[:, :1] + j[None, :]))


def _families(ctx, specs, Y, mean, yt):
    """The recorded arrays of every family on the context's current prediction."""
    ctx.solve_targets(Y, mean)
    out = {}
    for name, s in specs.items():
        kw = dict(plain=s["plain"], prior_kernel_id=s["prior_kid"])
        o = {}
        o["partial"] = ctx.aggregate_partial(s["family"], s["coef"], s["group"], s["G"])
        o["mu"], o["var"] = ctx.aggregate(s["family"], s["coef"], s["group"], s["G"], **kw)
        sc = ctx.scores(yt)
        o["scores"] = np.array([sc[k] for k in hipabi.SCORE_NAMES], dtype=np.float64)
        o["dmu"], o["dvar"] = ctx.aggregate_gradients(**kw)
        o["grad_partial"] = ctx.aggregate_gradients_partial()
        o["col_mu"], o["col_var"] = ctx.aggregate_columns(s["family"], s["coef"], s["group"], s["G"], **kw)
        o["col_dmu"], o["col_dvar"] = ctx.aggregate_columns_gradients(**kw)
        out.update({f"{name}/{k}": v for k, v in o.items()})
    return out


def _table(ctx, n_t, D):
    t = ac.small_table(n_t, D, 9200 + n_t + D)
    Y = columns(t["X"], t["y"])
    op, oi = t["obs_ptr"], t["obs_idx"]
    mean = np.stack([np.mean(Y[oi[op[l]:op[l + 1]]], axis=0) for l in range(ac.N_LEAVES)])
    mean[:, 0] = t["mean"]
    ac.small_predict(ctx, t)
    return _families(ctx, t["specs"], Y, mean, np.sin(3.0 * t["Xt"][:, 0]) + 0.7)


def _clamp(ctx):
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
    assert np.any(ctx.predict_fetch()[1] <= 0.0), "no leaf variance came out <= 0: the case shows nothing"
    specs = dict(mixture=ac.spec(ac.MIXTURE, coef=[1.0]), plain=ac.spec(ac.MIXTURE, coef=[1.0], plain=True))
    return _families(ctx, specs, columns(X, y), np.zeros((1, Q)), 0.8e-3 * Xt[:, 0])


def _failed_leaf(ctx):
    n0, n1, nt = 140, 100, 9
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Xt = np.asfortranarray(np.linspace(0.05, 0.95, nt).reshape(-1, 1))
    ctx.set_train(X, y)
    ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
    ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
    ctx.set_hyper(1, 0, [np.log(0.3), 0.0, np.log(0.1)])
    _, info, _ = ctx.fit()
    assert info[0] != 0 and info[1] == 0
    ctx.set_test(Xt, [0, 6, 6 + nt], np.concatenate([np.arange(6), np.arange(nt)]))
    ctx.predict_run()
    specs = dict(mixture=ac.spec(ac.MIXTURE, coef=[0.4, 0.6]), plain=ac.spec(ac.MIXTURE, coef=[0.4, 0.6], plain=True),
                 poe=ac.spec(ac.POE, coef=[1.0, 1.0]), gpoe=ac.spec(ac.GPOE, coef=[0.5, 0.5]),
                 rbcm=ac.spec(ac.RBCM, group=[0, 1], G=2, prior_kid=1))
    return _families(ctx, specs, columns(X, y), np.array([[0.0] * Q, [0.2, 0.3, 0.4]]), np.sin(3.0 * Xt[:, 0]))


def _make_cases():
    cases = {f"table/{n_t}x{D}": (lambda ctx, n_t=n_t, D=D: _table(ctx, n_t, D)) for n_t, D in TABLES}
    cases["clamp"] = _clamp
    cases["failed_leaf"] = _failed_leaf
    return cases


CASES = _make_cases()      # name -> f(ctx) -> {"<family>/<array>": float64 array}


def run(name):
    """The arrays of one case, from a context of its own."""
    ctx = hipabi.Context(0)
    try:
        return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in CASES[name](ctx).items()}
    finally:
        ctx.close()
