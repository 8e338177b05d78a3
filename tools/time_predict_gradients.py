"""Device time of dsmgp_predict_gradients beside the standalone prediction sweep (dsmgp_predict_run) of the same shape:
one JSON line per shape to stdout and to profiles/predict_grad_time.jsonl.
Per shape (single IsoSE GP, n training rows, n_t test rows, D dimensions): fit, register the rows, one standalone
predict_run (the sweep K_tn L^-T; its device seconds), then one warm-up and `--reps` calls of predict_gradients with and
without the variance half.  The first full call after a fit also inverts L (the L^-T arena) and materialises alpha: it is
reported separately as `first`.
    python tools/time_predict_gradients.py [--reps 5] [--shapes 1500x400x8,4096x4096x4,4096x512x4]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="1500x400x8,4096x4096x4,4096x512x4")
    args = ap.parse_args()
    ctx = hipabi.Context(0)
    out = open(os.path.join(ROOT, "profiles", "predict_grad_time.jsonl"), "a", encoding="utf-8")
    for shape in args.shapes.split(","):
        n, nt, D = (int(v) for v in shape.split("x"))
        X, y, Xt = dsm.regression_data(n, D, n_test=nt, seed=20202)
        ctx.set_train(X, y)
        ctx.set_leaves([0, n], np.arange(n), [0], [float(np.mean(y))])
        ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))
        ctx.set_joint(0)
        _, info, _ = ctx.fit()
        assert info[0] == 0
        ctx.set_test(Xt, [0, nt], np.arange(nt))
        t_sweep = ctx.predict_run()                     # standalone: K_tn tiles + sweep + finish
        ctx.predict_gradients()
        first = ctx.grad_seconds                        # with the inversion of L and alpha
        full, mean_only = [], []
        for _ in range(args.reps):
            ctx.predict_gradients()
            full.append(ctx.grad_seconds)
            ctx.predict_gradients(want_var=False)
            mean_only.append(ctx.grad_seconds)
        rec = dict(device=ctx.device_name(), kind="IsoSE", n=n, nt=nt, D=D, predict_run_standalone=t_sweep, first=first,
                   full=stats(full), mean_only=stats(mean_only), flops_B=2.0 * n * n / 2 * nt, kernel_derivatives=float(n) * nt * D)
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
    out.close()
    ctx.close()


if __name__ == "__main__":
    main()
