"""Host time of dsmgp_mll_columns_gradients and dsmgp_loo_columns_gradients: the wall-clock of the call minus the device seconds
it reports, i.e. the task lists these two entry points rebuild and upload on every call, the downloads and the host reduction.
On the headline model of the benchmark (N = 100k, D = 8, depth 2) and on its depth-4 leaf table (18,461 leaves), Q = 8 target
columns.  One JSON line per config on stdout (and appended to --out when given).

Method: one fit and one solve_targets, one warm-up call of each entry point (it fills the L^-T arena and sizes the buffers), then
`--reps` calls of each on the same fit, alternating; every figure is the median / min / max over the repetitions, in seconds.
No threshold is asserted: for an A/B of two libraries compare the medians of one with the min-max spread of the other.
    python tools/time_columns_host.py [--reps 7] [--Q 8] [--configs dsmgp_n100k_d8,dsmgp_n100k_d8_depth4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import deepstructuredmixtures_amd as dsm  # noqa: E402


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--Q", type=int, default=8)
    ap.add_argument("--configs", default="dsmgp_n100k_d8,dsmgp_n100k_d8_depth4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    Q = args.Q
    for config in args.configs.split(","):
        m, X, y, _, _, _ = bench.build_model(config, 0, 1, 0)
        dsm.fit(m)
        ctx = m.ctx
        stride = max(lf.kernel.nparams() + 1 for lf in m.leaves)
        rng = np.random.default_rng(11)
        Y = np.asfortranarray(y[:, None] * (1.0 + 0.1 * np.arange(Q))[None, :] + 0.05 * rng.standard_normal((y.size, Q)))
        ctx.solve_targets(Y)                # (column means: the ABI's zeros; the host time does not depend on them)
        host = {"targets_gradients": [], "loo_targets_gradients": []}
        dev = {"targets_gradients": [], "loo_targets_gradients": []}
        for it in range(args.reps + 1):
            for name in host:
                t0 = time.perf_counter()
                getattr(ctx, name)(stride)
                wall = time.perf_counter() - t0
                sec = getattr(ctx, name + "_seconds")
                if it:
                    host[name].append(wall - sec)
                    dev[name].append(sec)
        rec = dict(what="columns_host_time", config=config, device=ctx.device_name(), L=m.L, N=int(X.shape[0]), Q=Q, reps=args.reps)
        for name in host:
            rec[name + "_host"] = stats(host[name])
            rec[name + "_device"] = stats(dev[name])
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as out:
                out.write(line + "\n")
        ctx.close()


if __name__ == "__main__":
    main()
