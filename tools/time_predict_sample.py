"""Time of joint posterior draws on the device (dsmgp_predict_sample) beside the host path they replace (predict_cov download,
np.linalg.cholesky, the product), on
  * the single GP n = 4096, D = 4, IsoSE (config 2's shape) with n_t = 1024, 4096, 10000 test rows,
  * the headline model of the benchmark (N = 100k, D = 8, depth 2) with its 10,000 candidates,
  * the depth-4 model with the same candidates,
each with S = 1 and S = 64 draws.  Appends JSON lines to profiles/predict_sample_time.jsonl.

Method (warm-up, repeats, spread): one warm-up pass, then `--reps` passes (default 3); every figure is median / min / max.
`--mode device`: per pass one call that factorises (the tag alternates between two jitters, so the factors are never current) and a
second call on the cached factors with new normals.  Recorded: the device seconds of the first call split into forming Sigma (with
the uploads of the task lists), the factorisation and the draws (dsmgp_predict_sample_seconds), the device seconds of the cached
call, the wall-clock of both Context.predict_sample calls (the check of eps, staging, copies and synchronisation included), and for a
single GP the f64 rate of the factorisation on n_t^3 / 3 flops beside the chip's 78.6 TFLOP/s.
`--mode host`: the wall-clock of the parent commit's path per leaf -- Context.predict_cov (device work and the download of
n_t^2 doubles), np.linalg.cholesky of Sigma + 1e-8 I, the product with the normals -- summed over the leaves with routed rows; at
depth 4 timed on every `--leaf-stride`-th leaf with routed rows (default 64) and scaled by the ratio of sum n_t^2 over all
leaves to that over the sample (stated in the record).  It uses only calls that exist without dsmgp_predict_sample, so with
`--lib` pointing at a library built from the parent commit it measures the parent's path.
No threshold is asserted.
    python tools/time_predict_sample.py [--reps 3] [--mode device|host] [--cases gp1024,gp4096,gp10000,headline,depth4]
                                        [--leaf-stride 64] [--lib FILE] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import hipabi, datagen  # noqa: E402
from deepstructuredmixtures_amd import model as dmodel  # noqa: E402

SS = (1, 64)
PEAK_F64 = 78.6e12


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def time_device(ctx, S, reps):
    n = int(ctx.route_total)
    first = dict(sigma=[], factor=[], draws=[], total=[], wall=[])
    cached = dict(device=[], wall=[])
    for it in range(reps + 1):
        eps = datagen.normal(100 + it, 0, n * S).reshape((n, S), order="F")
        t0 = time.perf_counter()
        _, info = ctx.predict_sample(eps, with_noise=False, jitter=1e-8 * (1 + it % 2))     # never the tag of the factors at hand
        t1 = time.perf_counter()
        split, total = dict(ctx.sample_split_seconds), ctx.sample_seconds
        eps2 = datagen.normal(200 + it, 0, n * S).reshape((n, S), order="F")
        t2 = time.perf_counter()
        ctx.predict_sample(eps2, with_noise=False, jitter=1e-8 * (1 + it % 2))
        t3 = time.perf_counter()
        if it:
            for k in ("sigma", "factor", "draws"):
                first[k].append(split[k])
            first["total"].append(total)
            first["wall"].append(t1 - t0)
            cached["device"].append(ctx.sample_seconds)
            cached["wall"].append(t3 - t2)
    return dict(S=S, failed_leaves=int(np.count_nonzero(info)), first_call={k: stats(v) for k, v in first.items()},
                cached_call={k: stats(v) for k, v in cached.items()})


def time_host(ctx, ptr, S, reps, leaves):
    cov, chol, prod = [], [], []
    for it in range(reps + 1):
        a = b = c = 0.0
        for l in leaves:
            nt = int(ptr[l + 1] - ptr[l])
            eps = datagen.normal(100 + it, int(ptr[l]) * S, nt * S).reshape((nt, S), order="F")
            t0 = time.perf_counter()
            Sg = ctx.predict_cov(l, nt, with_noise=False)
            t1 = time.perf_counter()
            Sg[np.arange(nt), np.arange(nt)] += dmodel.EPS
            Lc = np.linalg.cholesky(Sg)
            t2 = time.perf_counter()
            Lc @ eps
            t3 = time.perf_counter()
            a, b, c = a + t1 - t0, b + t2 - t1, c + t3 - t2
        if it:
            cov.append(a)
            chol.append(b)
            prod.append(c)
    return dict(S=S, predict_cov_and_download=stats(cov), cholesky=stats(chol), product=stats(prod),
                total=stats([x + y + z for x, y, z in zip(cov, chol, prod)]))


def run_case(name, args, out):
    if name.startswith("gp"):
        nt = int(name[2:])
        X, y, _ = dsm.regression_data(4096, 4, n_test=16, seed=20202)
        Xt = datagen.uniform(20203, 0, nt * 4).reshape((nt, 4), order="F")
        gp = dsm.GaussianProcess(X, y, kernel=dsm.IsoSE(float(np.log(0.5)), 0.0), logNoise=float(np.log(0.1)), run_cholesky=True)
        dsm.prediction(gp, Xt)
        m = gp.model
        desc = dict(what="single_gp", n=4096, D=4, n_t=nt)
    else:
        X, y, Xt = dsm.regression_data(100_000, 8, seed=20204)
        m = dsm.buildDSMGP(X, y, 3, 4, M=200, D={"headline": 2, "depth4": 4}[name], kernel=dsm.IsoSE(float(np.log(0.3)), 0.0),
                           logNoise=float(np.log(0.1)), seed=20204, fit_now=False)
        dsm.fit(m)
        xt = dmodel._test_matrix(m, Xt)     # the rows through the host lists, as leaf_samples registers them, and the prediction
        rc = dmodel._routing(m, xt)
        m.ctx.set_test(xt, rc["lptr"], rc["lidx"])
        rc["uploaded"] = True
        m.ctx.predict_run()
        desc = dict(what="dsmgp_" + name, N=100_000, D=8, n_t=int(Xt.shape[0]), L=m.L)
    ctx = m.ctx
    ptr, _ = ctx.routes()
    cnt = np.diff(ptr)
    desc.update(mode=args.mode, lib=os.path.basename(hipabi.LIB_PATH), device=ctx.device_name(), route_total=int(ptr[-1]),
                leaves_with_rows=int(np.count_nonzero(cnt)), max_nt=int(cnt.max()), sum_nt2=float(np.sum(cnt.astype(np.float64) ** 2)),
                sum_nt3_over_3=float(np.sum(cnt.astype(np.float64) ** 3) / 3.0))
    for S in SS:
        if args.mode == "device":
            rec = dict(desc, **time_device(ctx, S, args.reps))
            rec["factor_TFLOPs"] = desc["sum_nt3_over_3"] / rec["first_call"]["factor"]["median"] * 1e-12
            rec["factor_fraction_of_peak"] = rec["factor_TFLOPs"] * 1e12 / PEAK_F64
        else:
            routed = [int(l) for l in np.nonzero(cnt)[0]]
            leaves = routed[::args.leaf_stride] if name == "depth4" else routed
            scale = desc["sum_nt2"] / float(np.sum(cnt[leaves].astype(np.float64) ** 2))
            rec = dict(desc, leaves_timed=len(leaves), scale_to_all_leaves=scale, **time_host(ctx, ptr, S, args.reps, leaves))
            rec["total_scaled_median"] = rec["total"]["median"] * scale
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", default="device", choices=["device", "host"])
    ap.add_argument("--cases", default="gp1024,gp4096,gp10000,headline,depth4")
    ap.add_argument("--leaf-stride", type=int, default=64)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_sample_time.jsonl"))
    args = ap.parse_args()
    if args.lib:
        hipabi.LIB_PATH = os.path.abspath(args.lib)
        if args.mode == "host":     # a library of the parent commit does not export the new symbols, and this mode calls none
            for name in [n for n in hipabi.SIGNATURES if n.startswith(("dsmgp_predict_sample", "dsmgp_predict_cov_factor"))]:
                del hipabi.SIGNATURES[name]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        for name in args.cases.split(","):
            run_case(name, args, out)


if __name__ == "__main__":
    main()
