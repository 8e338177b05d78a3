"""Device time of dsmgp_loo on a single GP (n = 4096, D = 4, IsoSE) and on the depth-4 leaf table of the benchmark (N = 100k,
D = 8, 18,461 leaves), beside its yardsticks on the same fit: the `grad_inverse` span (the L^-T sweep loo() runs when it cannot
reuse one) and the `grad_traces` span (frob_kernel reads the same bytes of L^-T as the row-sum pass, plus the per-leaf dots).
Per workload one JSON line: `loo_alone` = loo() right after a fit (builds L^-T), `loo_reused` = loo() after gradients() on the
same fit (reads it), each the median / min / max over `--reps` fits of the device time the call reports; `bytes` = the doubles of
L^-T the row-sum pass reads (sum over factor owners of the upper block triangle, padding columns left out), `gbps` = bytes over
the median reused time (which still holds the moments kernel and two launch gaps).
    python tools/time_loo.py [--reps 5] [--n 4096] [--skip-table]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import hipabi  # noqa: E402


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def rowsum_bytes(ns):
    """Doubles of L^-T the row-sum pass reads: per owner and 128-row tile t the columns 128 t .. n - 1 of its real rows."""
    tot = 0
    for n in ns:
        n = int(n)
        for t in range((n + 127) // 128):
            tot += min(128, n - 128 * t) * (n - 128 * t)
    return 8 * tot


def measure(what, ctx, ns_owner, stride, reps, extra):
    alone, reused, inv, traces = [], [], [], []
    for it in range(reps + 1):
        ctx.fit()
        ctx.loo()
        a = ctx.loo_seconds
        ctx.fit()
        ctx.gradients(stride)
        tm = ctx.timings()
        ctx.loo()
        if it:
            alone.append(a)
            reused.append(ctx.loo_seconds)
            inv.append(tm["grad_inverse"])
            traces.append(tm["grad_traces"])
    b = rowsum_bytes(ns_owner)
    print(json.dumps(dict(what=what, **extra, loo_alone=stats(alone), loo_reused=stats(reused), grad_inverse=stats(inv),
                          grad_traces=stats(traces), bytes=b, gbps=b / float(np.median(reused)) / 1e9)), flush=True)
    # a reused call that is not clearly cheaper means the inverse was built again: the per-fit flag is not working
    assert np.median(reused) < 0.5 * np.median(alone), (what, float(np.median(reused)), float(np.median(alone)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--skip-table", action="store_true")
    args = ap.parse_args()
    n, D = args.n, 4
    X, y, _ = dsm.regression_data(n, D, n_test=8, seed=20202)
    ctx = hipabi.Context(0)
    ctx.set_profile(2)          # per-launch timings: grad_inverse, grad_traces
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(np.mean(y))])
    ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))
    print(json.dumps(dict(device=ctx.device_name())), flush=True)
    measure("single_gp", ctx, [n], 3, args.reps, dict(n=n, D=D, kind="IsoSE"))
    ctx.close()
    if args.skip_table:
        return
    X, y, _ = dsm.regression_data(100_000, 8, seed=20204)
    m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=4, kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                       seed=20204, fit_now=False)
    dsm.fit(m)
    m.ctx.set_profile(2)
    owners = [lf.nobs for lf, op in zip(m.leaves, m.share_op) if op != 1]        # COPY leaves (op 1) read their source's sums
    measure("dsmgp_depth4", m.ctx, owners, 3, args.reps, dict(L=m.L, owners=len(owners), N=100_000, D=8, kind="IsoSE"))
    m.ctx.close()


if __name__ == "__main__":
    main()
