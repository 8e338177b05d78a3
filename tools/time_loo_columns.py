"""Device time of dsmgp_solve_targets + dsmgp_loo_columns_gradients at Q = 8 target columns on the headline model of the benchmark
(bench.build_model: N = 100k, D = 8, depth 2), beside what a user does WITHOUT them for the same result -- eight rounds of
set_train(y_q) + fit + dsmgp_loo_gradients -- and beside one dsmgp_loo_gradients on the same fit, its yardstick by the flop count
(n^3 / 3 for K_y^-1 plus n^3 for H H^T per leaf whatever Q is; the n^2 Q terms are small).  Appends JSON lines to
profiles/loo_columns_time.jsonl.

Method (warm-up, repeats, spread): one warm-up pass, then `--reps` passes; every figure is the median / min / max of the device
seconds the calls report (hipEvents around the device work).  Every timed call follows a fresh fit, so each one fills the L^-T
arena itself; `*_arena_valid` is the same call repeated on that fit, which reads the arena as it is.  The refit rounds are timed
one round (one column) per pass and multiplied by Q: the rounds are identical work, stated as such.  No threshold is asserted
beyond the figures themselves.
    python tools/time_loo_columns.py [--reps 5] [--Q 8] [--config dsmgp_n100k_d8]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd.tree import obs_table  # noqa: E402


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--Q", type=int, default=8)
    ap.add_argument("--config", default="dsmgp_n100k_d8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_columns_time.jsonl"))
    args = ap.parse_args()
    Q = args.Q
    m, X, y, _, _, _ = bench.build_model(args.config, 0, 1, 0)
    dsm.fit(m)
    ctx = m.ctx
    ptr, idx = obs_table(m.leaves)
    stride = max(lf.kernel.nparams() + 1 for lf in m.leaves)
    rng = np.random.default_rng(11)
    Y = np.asfortranarray(y[:, None] * (1.0 + 0.1 * np.arange(Q))[None, :] + 0.05 * rng.standard_normal((y.size, Q)))
    mean = np.zeros((m.L, Q))

    def setup():
        ctx.set_leaves(ptr, idx, [lf.kernelid for lf in m.leaves], [0.0] * m.L)
        ctx.set_sharing(None, None, None)
        m._push_hyper()

    ctx.set_train(m.x, m.y)
    setup()
    loo_grad, loo_grad_again, solve, first, again, moments, rounds = [], [], [], [], [], [], []
    for it in range(args.reps + 1):
        ctx.fit()
        ctx.loo_gradients(stride)
        a = ctx.loo_gradients_seconds
        ctx.loo_gradients(stride)
        b = ctx.loo_gradients_seconds
        ctx.fit()
        _, s = ctx.solve_targets(Y, mean)
        ctx.loo_targets_gradients(stride)
        f = ctx.loo_targets_gradients_seconds
        ctx.loo_targets_gradients(stride)
        g = ctx.loo_targets_gradients_seconds
        ctx.loo_targets()
        ctx.set_train(m.x, np.ascontiguousarray(Y[:, it % Q]))
        setup()
        _, _, sf = ctx.fit()
        ctx.loo_gradients(stride)
        r = sf + ctx.loo_gradients_seconds
        ctx.set_train(m.x, m.y)
        setup()
        if it:
            loo_grad.append(a)
            loo_grad_again.append(b)
            solve.append(s)
            first.append(f)
            again.append(g)
            moments.append(ctx.loo_targets_seconds)
            rounds.append(r)
    rec = dict(what="dsmgp_headline", config=args.config, device=ctx.device_name(), L=m.L, N=int(X.shape[0]), D=int(X.shape[1]), Q=Q,
               kind="IsoSE", sharing="none", reps=args.reps, solve_targets=stats(solve), loo_columns_gradients=stats(first),
               loo_columns_gradients_arena_valid=stats(again), loo_columns_arena_valid=stats(moments),
               new_total=float(np.median(solve) + np.median(first)), loo_gradients=stats(loo_grad),
               loo_gradients_arena_valid=stats(loo_grad_again), refit_round=stats(rounds),
               refit_total_Q=Q * float(np.median(rounds)))
    rec["new_over_one_loo_gradients"] = rec["new_total"] / rec["loo_gradients"]["median"]
    rec["refit_over_new"] = rec["refit_total_Q"] / rec["new_total"]
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        out.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
