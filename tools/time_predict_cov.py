"""Device time and f64 rate of dsmgp_predict_cov on the single-GP shape of config 2 (n = 4096, D = 4, IsoSE), beside its
yardstick: the contraction pass of the gradients (the same main loop, gemm_mainloop_v2, with a comparable per-element epilogue)
on the same n, and the register-only f64 MFMA probe as the ceiling.
Per nt: one warm-up call, then `--reps` calls; the seconds are the device time the call itself reports (hipEvents around the
launch).  Rates: `alg` = nt^2 n / seconds (the useful product), `exec` = nt (nt + 128) n / seconds (the lower tiles that ran,
2 flops per multiply-add).  Contraction: dsmgp_work_gradients' contraction flops (n^3 / 3) over the grad_contraction timing.
    python tools/time_predict_cov.py [--reps 7] [--n 4096] [--nt 4096,512]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--nt", default="4096,512")
    args = ap.parse_args()
    n, D = args.n, 4
    nts = [int(v) for v in args.nt.split(",")]
    X, y, Xt = dsm.regression_data(n, D, n_test=max(nts), seed=20202)
    ctx = hipabi.Context(0)
    ctx.set_profile(2)          # per-launch timings: grad_contraction
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [float(np.mean(y))])
    ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))
    _, info, _ = ctx.fit()
    assert info[0] == 0
    print(json.dumps(dict(device=ctx.device_name(), n=n, D=D, kind="IsoSE")), flush=True)
    # the yardstick: the contraction pass on the same n
    rates, secs = [], []
    for it in range(args.reps + 1):
        ctx.gradients(3)
        t = ctx.timings()["grad_contraction"]
        flops = ctx.work_gradients()[1]
        if it:
            secs.append(t)
            rates.append(flops / t / 1e12)
    print(json.dumps(dict(what="grad_contraction", flops=flops, seconds=stats(secs), tflops=stats(rates))), flush=True)
    probe = [ctx.probe_f64_mfma() for _ in range(3)]
    print(json.dumps(dict(what="probe_f64_mfma", tflops=stats(probe))), flush=True)
    for nt in nts:
        xt = np.asfortranarray(Xt[:nt])
        ctx.predict_leaves(xt, [0, nt], np.arange(nt))
        secs = []
        for it in range(args.reps + 1):
            ctx.predict_cov(0, nt, with_noise=False)
            if it:
                secs.append(ctx.cov_seconds)
        s = np.array(secs)
        ntp = (nt + 127) // 128 * 128
        alg, exe = float(nt) * nt * n, float(ntp) * (ntp + 128) * n
        print(json.dumps(dict(what="predict_cov", nt=nt, lower_tiles=(ntp // 128) * (ntp // 128 + 1) // 2, seconds=stats(s),
                              tflops_alg=stats(alg / s / 1e12), tflops_exec=stats(exe / s / 1e12))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
