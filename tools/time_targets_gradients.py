"""Device time of dsmgp_solve_targets + dsmgp_mll_columns_gradients at Q = 1, 8, 64 target columns on the single GP of n = 4096
(D = 4, IsoSE) and on the headline model of the benchmark (N = 100k, D = 8, depth 2), beside what a user does WITHOUT them for the
same result -- Q rounds of set_train(y_j) + fit + dsmgp_gradients -- and beside dsmgp_gradients alone.  Appends JSON lines to
profiles/targets_grad_time.jsonl.

Method (warm-up, repeats, spread): one warm-up pass, then `--reps` passes; every figure is the median / min / max of the device
seconds the calls report (hipEvents around the device work; dsmgp_gradients: the `gradients` slot of dsmgp_timings, which has
none for the alpha it completes first -- that is in `alpha`).  `--mode new` (default) times the new calls, each
targets_gradients once after a fit (it inverts) and once again (it reads the L^-T arena as it is); `--mode refit` uses only
calls that exist without them, so the same file runs on a checkout of the parent commit for an alternating series on one box;
`--mode both` alternates the two in one process.  `refit_total_Q` = Q times the median round (stated as such: the rounds are
identical work).  No threshold is asserted: the expectation from the flop counts is one dsmgp_gradients plus O(n^2 Q).
    python tools/time_targets_gradients.py [--reps 5] [--mode new|refit|both] [--skip-headline]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import hipabi  # noqa: E402

QS = (1, 8, 64)


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def columns(y, Q, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(y[:, None] * (1.0 + 0.1 * np.arange(Q))[None, :] + 0.05 * rng.standard_normal((y.size, Q)))


def time_gradients_alone(ctx, stride, reps):
    out = []
    for it in range(reps + 1):
        ctx.fit()
        ctx.gradients(stride)
        tm = ctx.timings()
        if it:
            out.append(tm["gradients"] + tm["alpha"])
    return out


def time_new(ctx, Y, mean, stride, reps):
    solve, first, again = [], [], []
    for it in range(reps + 1):
        ctx.fit()
        _, s = ctx.solve_targets(Y, mean)
        ctx.targets_gradients(stride)
        a = ctx.targets_gradients_seconds
        ctx.targets_gradients(stride)
        if it:
            solve.append(s)
            first.append(a)
            again.append(ctx.targets_gradients_seconds)
    return solve, first, again


def time_refit_round(ctx, X, ycol, setup, stride, reps):
    """One column the old way: new targets, a fit, the gradient pass."""
    out = []
    for it in range(reps + 1):
        ctx.set_train(X, ycol)
        setup()
        _, _, sf = ctx.fit()
        ctx.gradients(stride)
        tm = ctx.timings()
        if it:
            out.append(sf + tm["gradients"] + tm["alpha"])
    return out


def run(what, ctx, X, y, setup, stride, mode, reps, extra, out):
    ctx.set_train(X, y)
    setup()
    rec = dict(what=what, mode=mode, **extra, gradients_alone=stats(time_gradients_alone(ctx, stride, reps)))
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    for Q in QS:
        rec = dict(what=what, Q=Q, mode=mode, **extra)
        Y = columns(y, Q, 7 + Q)
        if mode in ("refit", "both"):
            r = time_refit_round(ctx, X, np.ascontiguousarray(Y[:, 0]), setup, stride, reps)
            rec.update(refit_round=stats(r), refit_total_Q=Q * float(np.median(r)))
        if mode in ("new", "both"):
            ctx.set_train(X, y)
            setup()
            solve, first, again = time_new(ctx, Y, np.zeros((ctx.L, Q)), stride, reps)
            rec.update(solve_targets=stats(solve), targets_gradients=stats(first), targets_gradients_arena_valid=stats(again),
                       new_total=float(np.median(solve) + np.median(first)))
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", default="new", choices=["new", "refit", "both"])
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets_grad_time.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")
    n, D = 4096, 4
    X, y, _ = dsm.regression_data(n, D, n_test=8, seed=20202)
    ctx = hipabi.Context(0)
    dev = ctx.device_name()

    def setup_gp():
        ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
        ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))

    run("single_gp", ctx, X, y, setup_gp, 3, args.mode, args.reps, dict(device=dev, n=n, D=D, kind="IsoSE"), out)
    ctx.close()
    if args.skip_headline:
        return
    X, y, _ = dsm.regression_data(100_000, 8, seed=20204)
    m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=2, kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                       seed=20204, fit_now=False)
    dsm.fit(m)
    c2 = m.ctx
    from deepstructuredmixtures_amd.tree import obs_table
    ptr, idx = obs_table(m.leaves)

    def setup_model():
        c2.set_leaves(ptr, idx, [lf.kernelid for lf in m.leaves], [0.0] * m.L)
        c2.set_sharing(None, None, None)
        m._push_hyper()

    run("dsmgp_headline", c2, m.x, m.y, setup_model, 3, args.mode, args.reps,
        dict(device=dev, L=m.L, N=100_000, D=8, kind="IsoSE", sharing="none"), out)
    c2.close()


if __name__ == "__main__":
    main()
