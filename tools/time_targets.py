"""Device time of dsmgp_solve_targets + dsmgp_predict_targets at Q = 1, 8, 64 target columns on the single GP of n = 4096
(D = 4, IsoSE) and on the headline model of the benchmark (N = 100k, D = 8, depth 2), beside what a user does WITHOUT them for the
same result: one round of set_train + fit + predict_run per column.  Appends JSON lines to profiles/targets_time.jsonl.

Method (warm-up, repeats, spread): one warm-up pass, then `--reps` passes; every figure is the median / min / max of the device
seconds the calls report (hipEvents around the device work).  `--mode new` (default) times the new calls; `--mode refit` uses
only calls that exist without them, so the same file runs on a checkout of the parent commit for an alternating series
(new, refit, new, refit ... on one box); `--mode both` alternates the two in one process.  A round of the refit path is timed
`--reps` times and reported per round; `refit_total_Q` = Q times the median round (stated as such: the rounds are identical work).
`factor_bytes` = the doubles of the factor the sweep reads (block lower triangle of every leaf, once per call whatever Q is),
`gbps` = factor_bytes over the median solve time, to be read against the HBM figure of the micro-architecture guide.
The one condition that follows from the flop counts (2 n^2 Q against Q n^3 / 3): at Q = 8 the new path must take less time than
the eight refits it replaces -- asserted in `--mode both`.
    python tools/time_targets.py [--reps 5] [--mode new|refit|both] [--skip-headline]"""
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


def factor_bytes(ns):
    tot = 0
    for n in ns:
        nb = (int(n) + 127) // 128
        tot += nb * (nb + 1) // 2 * 128 * 128
    return 8 * tot


def columns(y, Q, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(y[:, None] * (1.0 + 0.1 * np.arange(Q))[None, :] + 0.05 * rng.standard_normal((y.size, Q)))


def time_new(ctx, Y, mean, reps):
    solve, pred = [], []
    for it in range(reps + 1):
        _, s = ctx.solve_targets(Y, mean)
        ctx.predict_targets()
        if it:
            solve.append(s)
            pred.append(ctx.predict_targets_seconds)
    return solve, pred


def time_refit_round(ctx, X, ycol, setup, reps):
    """One column the old way: new targets, a fit, the prediction sweep."""
    out = []
    for it in range(reps + 1):
        ctx.set_train(X, ycol)
        setup()
        _, _, sf = ctx.fit()
        sp = ctx.predict_run()
        if it:
            out.append(sf + sp)
    return out


def run(what, ctx, X, y, ns, setup, mode, reps, extra, out):
    for Q in QS:
        rec = dict(what=what, Q=Q, mode=mode, **extra, factor_bytes=factor_bytes(ns))
        Y = columns(y, Q, 7 + Q)
        if mode in ("refit", "both"):
            r = time_refit_round(ctx, X, np.ascontiguousarray(Y[:, 0]), setup, reps)
            rec.update(refit_round=stats(r), refit_total_Q=Q * float(np.median(r)))
        if mode in ("new", "both"):
            ctx.set_train(X, y)
            setup()
            ctx.fit()
            ctx.predict_run()
            solve, pred = time_new(ctx, Y, np.zeros((ctx.L, Q)), reps)
            rec.update(solve_targets=stats(solve), predict_targets=stats(pred),
                       new_total=float(np.median(solve) + np.median(pred)), gbps=rec["factor_bytes"] / float(np.median(solve)) / 1e9)
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        if mode == "both" and Q == 8:
            assert rec["new_total"] < rec["refit_total_Q"], (what, rec["new_total"], rec["refit_total_Q"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", default="new", choices=["new", "refit", "both"])
    ap.add_argument("--skip-headline", action="store_true")
    args = ap.parse_args()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    out = open(os.path.join(ROOT, "profiles", "targets_time.jsonl"), "a")
    n, D = 4096, 4
    X, y, Xt = dsm.regression_data(n, D, n_test=512, seed=20202)
    ctx = hipabi.Context(0)
    ctx.set_joint(False)        # fit and the prediction sweep timed apart, the sweep standalone in both paths
    dev = ctx.device_name()

    def setup_gp():
        ctx.set_leaves([0, n], np.arange(n), [0], [0.0])
        ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))
        ctx.set_test(Xt, [0, Xt.shape[0]], np.arange(Xt.shape[0]))

    run("single_gp", ctx, X, y, [n], setup_gp, args.mode, args.reps, dict(device=dev, n=n, D=D, n_t=512, kind="IsoSE"), out)
    ctx.close()
    if args.skip_headline:
        return
    X, y, Xt = dsm.regression_data(100_000, 8, seed=20204)
    m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=2, kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                       seed=20204, fit_now=False)
    dsm.fit(m)
    c2 = m.ctx
    c2.set_joint(False)
    from deepstructuredmixtures_amd import tree as ptree
    from deepstructuredmixtures_amd.tree import obs_table
    ptr, idx = obs_table(m.leaves)
    rptr, ridx = ptree.route(m.root, Xt)

    def setup_model():
        c2.set_leaves(ptr, idx, [lf.kernelid for lf in m.leaves], [0.0] * m.L)
        c2.set_sharing(None, None, None)
        m._push_hyper()
        c2.set_test(Xt, rptr, ridx)

    run("dsmgp_headline", c2, m.x, m.y, [lf.nobs for lf in m.leaves], setup_model, args.mode, args.reps,
        dict(device=dev, L=m.L, N=100_000, D=8, n_t=int(Xt.shape[0]), kind="IsoSE", sharing="none"), out)
    c2.close()


if __name__ == "__main__":
    main()
