"""Device time of dsmgp_solve_targets + dsmgp_predict_columns_gradients at Q = 1, 8, 64 target columns on the headline model of the
benchmark (N = 100k, D = 8, depth 2) and on the depth-4 model, each with its benchmark test set (N / 10 rows, routed by the tree),
beside what a user does WITHOUT the call for the same result -- Q rounds of set_train(y_q) + fit + predict_run +
predict_gradients(want_var=False) -- and, at Q = 1, beside dsmgp_predict_gradients(want_var=False) on the same context.  Appends
JSON lines to profiles/targets_inputgrad_time.jsonl.

Method (warm-up, repeats, spread): one warm-up pass, then `--reps` passes (default 3); every figure is the median / min / max of
the device seconds the calls report (hipEvents around the device work).  `--mode new` (default) times the new call, once after a
fit (it inverts L and forms A) and once again (it reads the L^-T arena as it is; A is formed again); `--mode refit` uses only
calls that exist without it, so the same file runs on a checkout of the parent commit with the parent's library, the way
tools/time_targets_gradients.py runs its rounds.  `refit_total_Q` = Q times the median round (stated as such: the rounds are
identical work).  No threshold is asserted.
    python tools/time_targets_inputgrad.py [--reps 3] [--mode new|refit] [--models headline,depth4] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import tree as ptree  # noqa: E402

QS = (1, 8, 64)
MODELS = {"headline": 2, "depth4": 4}


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def columns(y, Q, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(y[:, None] * (1.0 + 0.1 * np.arange(Q))[None, :] + 0.05 * rng.standard_normal((y.size, Q)))


def time_refit_round(ctx, X, ycol, setup, reps):
    """One column the old way: new targets, a fit, the prediction of the registered rows, the mean-only input gradients."""
    out = []
    for it in range(reps + 1):
        ctx.set_train(X, ycol)
        setup()
        _, _, sf = ctx.fit()
        sp = ctx.predict_run()
        ctx.predict_gradients(want_var=False)
        if it:
            out.append(sf + sp + ctx.grad_seconds)
    return out


def time_new(ctx, Y, mean, reps):
    solve, first, again, single = [], [], [], []
    for it in range(reps + 1):
        ctx.fit()
        ctx.predict_run()
        _, s = ctx.solve_targets(Y, mean)
        ctx.predict_targets_gradients()
        a = ctx.predict_targets_gradients_seconds
        ctx.predict_targets_gradients()
        b = ctx.predict_targets_gradients_seconds
        ctx.predict_gradients(want_var=False)           # (materialises alpha)
        ctx.predict_gradients(want_var=False)
        if it:
            solve.append(s)
            first.append(a)
            again.append(b)
            single.append(ctx.grad_seconds)
    return solve, first, again, single


def run(what, ctx, X, y, setup, mode, reps, extra, out):
    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    ctx.set_train(X, y)
    setup()
    if mode == "refit":
        r = time_refit_round(ctx, X, np.ascontiguousarray(columns(y, 1, 8)[:, 0]), setup, reps)
        emit(dict(what=what, mode=mode, **extra, refit_round=stats(r), refit_total_Q={str(Q): Q * float(np.median(r)) for Q in QS}))
        return
    for Q in QS:
        solve, first, again, single = time_new(ctx, columns(y, Q, 7 + Q), np.zeros((ctx.L, Q)), reps)
        emit(dict(what=what, Q=Q, mode=mode, **extra, solve_targets=stats(solve), predict_targets_gradients=stats(first),
                  predict_targets_gradients_arena_valid=stats(again), predict_gradients_mean_only=stats(single),
                  new_total=float(np.median(solve) + np.median(first))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", default="new", choices=["new", "refit"])
    ap.add_argument("--models", default="headline,depth4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_inputgrad_time.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")
    X, y, Xt = dsm.regression_data(100_000, 8, seed=20204)
    for name in args.models.split(","):
        m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=MODELS[name], kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                           seed=20204, fit_now=False)
        dsm.fit(m)
        ctx = m.ctx
        optr, oidx = ptree.obs_table(m.leaves)
        rptr, ridx = ptree.route(m.root, Xt)

        def setup():
            ctx.set_leaves(optr, oidx, [lf.kernelid for lf in m.leaves], [0.0] * m.L)
            ctx.set_sharing(None, None, None)
            m._push_hyper()
            ctx.set_test(Xt, rptr, ridx)

        run("dsmgp_" + name, ctx, m.x, m.y, setup, args.mode, args.reps,
            dict(device=ctx.device_name(), L=m.L, N=100_000, D=8, n_t=int(Xt.shape[0]), route_total=int(rptr[-1]), kind="IsoSE",
                 sharing="none"), out)
        ctx.close()
    out.close()


if __name__ == "__main__":
    main()
