"""Device time of fit, gradient pass and predict for IsoSE, ArdSEProduct, IsoMatern52 and ArdMatern52 at equal length-scales,
on the headline tree (buildDSMGP N = 100k, D = 8, M = 200, depth 2), on the config-3 shape (buildPoE K = 8, M = 200, N = 50k,
D = 8: 128 experts of n ~ 391) and on the depth-4 tree (bench.py's dsmgp_n100k_d8_depth4: buildDSMGP N = 100k, D = 8, K = 3,
V = 4, M = 200, depth 4).  Per kind: one warm-up pass, then the median and range over `--reps` passes of the library's own event
timings (total_fit, gradients, grad_contraction) and the wall clock of predict (a blocking call, the same test rows every pass).
    python tools/time_matern.py [--reps 5] [--shapes headline,config3,depth4]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepstructuredmixtures_amd as dsm  # noqa: E402


def kinds(D, logl, logs):
    return (("IsoSE", dsm.IsoSE(logl, logs)),
            ("ArdSEProduct", dsm.ArdSEProduct(np.full(D, logl), logs)),
            ("IsoMatern52", dsm.IsoMatern52(logl, logs)),
            ("ArdMatern52", dsm.ArdMatern52(np.full(D, logl), logs)))


def run(shape, build, X, y, Xt, reps):
    out = {}
    for name, kern in kinds(X.shape[1], np.log(0.3), 0.0):
        m = build(kern)
        rows = []
        for it in range(reps + 1):
            dsm.fit(m)
            t = dict(m.ctx.timings())
            dsm.updategradients(m)
            g = dict(m.ctx.timings())
            t0 = time.perf_counter()
            dsm.predict(m, Xt)
            tp = time.perf_counter() - t0
            if it:
                rows.append((t["total_fit"], g["gradients"], g["grad_contraction"], tp))
        a = np.array(rows)
        out[name] = {k: dict(median=float(np.median(a[:, i])), min=float(a[:, i].min()), max=float(a[:, i].max()))
                     for i, k in enumerate(("fit", "gradients", "grad_contraction", "predict"))}
        print(json.dumps(dict(shape=shape, kind=name, leaves=m.L, **{k: round(v["median"], 5) for k, v in out[name].items()})),
              flush=True)
        m.ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="headline,config3,depth4")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    res = {}
    X, y, Xt = dsm.regression_data(100000, 8, n_test=10000, seed=20204)
    if "headline" in shapes:
        res["headline"] = run("headline", lambda k: dsm.buildDSMGP(X, y, 3, 4, M=200, D=2, kernel=k, logNoise=np.log(0.1),
                                                                   seed=20204), X, y, Xt, args.reps)
    if "depth4" in shapes:
        res["depth4"] = run("depth4", lambda k: dsm.buildDSMGP(X, y, 3, 4, M=200, D=4, kernel=k, logNoise=np.log(0.1), seed=20204),
                            X, y, Xt, args.reps)
    if "config3" in shapes:
        X3, y3, Xt3 = dsm.regression_data(50000, 8, n_test=5000, seed=20205)
        mf = dsm.ConstMean(float(np.mean(y3)))
        res["config3"] = run("config3", lambda k: dsm.buildPoE(X3, y3, 8, M=200, kernel=k, meanFun=mf, logNoise=np.log(0.1),
                                                               seed=20205), X3, y3, Xt3, args.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
