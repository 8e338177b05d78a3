"""Device time of fit, gradient pass and LOO-gradient pass for ArdSEProduct, IsoRQ and ArdRQ at equal length-scales on the
config-3 shape (buildPoE K = 8, M = 200, N = 50k, D = 8: 128 experts of n ~ 391) and on the headline tree (buildDSMGP N = 100k,
D = 8, M = 200, depth 2): what the log1p of the rational quadratic Gram epilogue and the extra contraction sum cost.  Per kind:
one warm-up pass, then the median and range over `--reps` passes of the library's own event timings.  One JSON line per shape and
kind is appended to profiles/rq_time.jsonl.
    python tools/time_rq.py [--reps 5] [--shapes config3,headline]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepstructuredmixtures_amd as dsm  # noqa: E402


def kinds(D, logl, logs):
    return (("ArdSEProduct", dsm.ArdSEProduct(np.full(D, logl), logs)),
            ("IsoRQ", dsm.IsoRQ(logl, np.log(2.0), logs)),
            ("ArdRQ", dsm.ArdRQ(np.full(D, logl), np.log(2.0), logs)))


def run(shape, build, reps, out):
    for name, kern in kinds(8, np.log(0.3), 0.0):
        m = build(kern)
        rows = []
        for it in range(reps + 1):
            dsm.fit(m)
            t = dict(m.ctx.timings())
            dsm.updategradients(m)
            g = dict(m.ctx.timings())
            dsm.updategradients(m, objective="loo")
            if it:
                rows.append((t["total_fit"], g["gradients"], g["grad_contraction"], m.ctx.loo_gradients_seconds))
        a = np.array(rows)
        rec = dict(shape=shape, kind=name, leaves=m.L, reps=reps)
        for i, k in enumerate(("fit", "gradients", "grad_contraction", "loo_gradients")):
            rec[k] = dict(median=float(np.median(a[:, i])), min=float(a[:, i].min()), max=float(a[:, i].max()))
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        m.ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="config3,headline")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    with open(os.path.join(ROOT, "profiles", "rq_time.jsonl"), "a") as out:
        if "config3" in shapes:
            X3, y3, _ = dsm.regression_data(50000, 8, n_test=16, seed=20205)
            mf = dsm.ConstMean(float(np.mean(y3)))
            run("config3", lambda k: dsm.buildPoE(X3, y3, 8, M=200, kernel=k, meanFun=mf, logNoise=np.log(0.1), seed=20205),
                args.reps, out)
        if "headline" in shapes:
            X, y, _ = dsm.regression_data(100000, 8, n_test=16, seed=20204)
            run("headline", lambda k: dsm.buildDSMGP(X, y, 3, 4, M=200, D=2, kernel=k, logNoise=np.log(0.1), seed=20204),
                args.reps, out)


if __name__ == "__main__":
    main()
