"""Device time of dsmgp_loo_gradients on the two workloads of profiles/loo_time.jsonl -- a single GP (n = 4096, D = 4, IsoSE) and
the depth-4 leaf table of the benchmark (N = 100k, D = 8, 18,461 leaves) -- beside its yardsticks from the same process and fit:
the `grad_inverse` and `grad_contraction` spans of gradients(), which run on the same main loop.  Per workload one JSON line,
appended to profiles/loo_grad_time.jsonl: `alone` = loo_gradients() right after a fit (builds L^-T), `reused` = loo_gradients()
after gradients() on the same fit (reads it), each the median / min / max over `--reps` fits of the device time the call
reports; `ratio_alone` = alone / (grad_inverse + grad_contraction) (2.5 by the flop count: n^3/3 + n^3/3 + n^3 against
n^3/3 + n^3/3), `ratio_reused` = reused / grad_contraction (4 by the flop count).
    python tools/time_loo_gradients.py [--reps 5] [--n 4096] [--skip-table]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import hipabi  # noqa: E402


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def measure(what, ctx, stride, reps, extra, out):
    alone, reused, inv, dot = [], [], [], []
    for it in range(reps + 1):
        ctx.fit()
        ctx.loo_gradients(stride)
        a = ctx.loo_gradients_seconds
        ctx.fit()
        ctx.gradients(stride)
        tm = ctx.timings()
        ctx.loo_gradients(stride)
        if it:
            alone.append(a)
            reused.append(ctx.loo_gradients_seconds)
            inv.append(tm["grad_inverse"])
            dot.append(tm["grad_contraction"])
    line = json.dumps(dict(what=what, **extra, alone=stats(alone), reused=stats(reused), grad_inverse=stats(inv),
                           grad_contraction=stats(dot),
                           ratio_alone=float(np.median(alone) / (np.median(inv) + np.median(dot))),
                           ratio_reused=float(np.median(reused) / np.median(dot))))
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--skip-table", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_grad_time.jsonl"))
    args = ap.parse_args()
    n, D = args.n, 4
    with open(args.out, "a") as out:
        X, y, _ = dsm.regression_data(n, D, n_test=8, seed=20202)
        ctx = hipabi.Context(0)
        ctx.set_profile(2)          # per-launch timings: grad_inverse, grad_contraction
        ctx.set_train(X, y)
        ctx.set_leaves([0, n], np.arange(n), [0], [float(np.mean(y))])
        ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))
        line = json.dumps(dict(device=ctx.device_name()))
        print(line, flush=True)
        out.write(line + "\n")
        measure("single_gp", ctx, 3, args.reps, dict(n=n, D=D, kind="IsoSE"), out)
        ctx.close()
        if args.skip_table:
            return
        X, y, _ = dsm.regression_data(100_000, 8, seed=20204)
        m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=4, kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                           seed=20204, fit_now=False)
        dsm.fit(m)
        m.ctx.set_profile(2)
        measure("dsmgp_depth4", m.ctx, 3, args.reps, dict(L=m.L, N=100_000, D=8, kind="IsoSE"), out)
        m.ctx.close()


if __name__ == "__main__":
    main()
