"""Time of the aggregation of the input gradients over the leaves of every test row, on the device (dsmgp_aggregate_gradients)
and on the host (what predict_gradients(model, x) does by default), on the headline model of the benchmark (N = 100k, D = 8,
depth 2) and on the depth-4 model, each with its benchmark test set (N / 10 rows).  Appends JSON lines to
profiles/aggregate_gradients_time.jsonl.

Method (warm-up, repeats, spread): one warm-up pass, then `--reps` passes (default 3); every figure is the median / min / max.
`--mode device`: the device seconds the call reports (hipEvents around the device work) with the per-entry gradients current
(`sums`: the partial-sum kernel alone, one event interval -- at 14 us it is near the events' resolution; the finish kernel is
not timed) and after a fresh predict_run (`with_entries`: the per-entry gradients are made first),
the wall-clock of Context.aggregate_gradients (kernels, copy of 2 n_t D doubles, synchronisation) and of the whole model call;
beside them the bytes of the per-entry arrays the reduction gathers, 8 (2 D + 2) route_total, and that over `sums`.
`--mode host`: the wall-clock of the host step entry by entry -- the fetches of mu, var, dmu, dvar (the device work of
predict_gradients is reported apart and is not part of the step), the entry lists, aggregate_input_gradients.  It uses only
calls that exist without the device aggregation, so with `--lib` pointing at a library built from the parent commit it measures
the parent's path.
The target columns, Q = 1, 8, 64 (`columns` records): `--mode device` gives the device seconds of aggregate_columns and of
aggregate_columns_gradients with the per-entry arrays current (the aggregation kernels alone), the bytes of the per-entry
arrays they gather -- 8 (Q + 1) route_total and 8 (D Q + D + Q + 1) route_total -- and the rate of the two together;
`--mode host` gives the wall-clock of the host step of predict_targets_gradients: the fetches of the four per-entry arrays,
the entry lists, and the two per-column loops (predict_targets' `_aggregate_host` and aggregate_input_gradients), the loops
timed on the first min(Q, 4) columns and stated for Q columns as Q times the median column (the columns are identical work).
No threshold is asserted.
    python tools/time_aggregate_gradients.py [--reps 3] [--mode device|host] [--models headline,depth4] [--lib FILE] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import hipabi  # noqa: E402
from deepstructuredmixtures_amd import model as dmodel  # noqa: E402

MODELS = {"headline": 2, "depth4": 4}
QS = (1, 8, 64)


def stats(a):
    a = np.asarray(a, dtype=np.float64)
    return dict(median=float(np.median(a)), min=float(a.min()), max=float(a.max()))


def time_device(m, Xt, reps):
    ctx = m.ctx
    _, _, _, _, plain, prior = dmodel._aggregation_spec(m)
    kid = prior.kernelid if prior else 0
    sums, with_entries, wall_call, wall_model = [], [], [], []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        dsm.predict_gradients(m, Xt, aggregate="device")        # a fresh predict_run: the per-entry gradients are made first
        t1 = time.perf_counter()
        a = ctx.agg_gradients_seconds
        t2 = time.perf_counter()
        ctx.aggregate_gradients(plain=plain, prior_kernel_id=kid)
        t3 = time.perf_counter()
        if it:
            with_entries.append(a)
            sums.append(ctx.agg_gradients_seconds)
            wall_call.append(t3 - t2)
            wall_model.append(t1 - t0)
    return dict(sums=stats(sums), with_entries=stats(with_entries), wall_aggregate_gradients=stats(wall_call),
                wall_predict_gradients_device=stats(wall_model))


def time_host(m, Xt, reps):
    ctx = m.ctx
    xt = np.asfortranarray(Xt)
    n_t = xt.shape[0]
    family, coef, group, G, plain, prior = dmodel._aggregation_spec(m)
    fetch, lists, agg, dev = [], [], [], []
    for it in range(reps + 1):
        dsm.predict(m, xt)
        rc = dmodel._routing(m, xt)
        ptr, idx = rc["lptr"], rc["lidx"]
        t0 = time.perf_counter()
        mu_l, var_l = ctx.predict_fetch()
        dmu_l, dvar_l = ctx.predict_gradients()
        t1 = time.perf_counter()
        ent = [[] for _ in range(n_t)]
        for l in range(len(ptr) - 1):
            for k in range(int(ptr[l]), int(ptr[l + 1])):
                ent[int(idx[k])].append((l, k))
        t2 = time.perf_counter()
        dsm.aggregate_input_gradients(family, mu_l, var_l, dmu_l, dvar_l, ent, coef=coef, group=group, G=G, plain=plain)
        t3 = time.perf_counter()
        if it:
            dev.append(ctx.grad_seconds)
            fetch.append(t1 - t0 - ctx.grad_seconds)
            lists.append(t2 - t1)
            agg.append(t3 - t2)
    total = [a + b + c for a, b, c in zip(fetch, lists, agg)]
    return dict(fetch_entries=stats(fetch), entry_lists=stats(lists), aggregate_input_gradients=stats(agg), host_step=stats(total),
                predict_gradients_device=stats(dev))


def columns(y, Q, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(y[:, None] * (1.0 + 0.1 * np.arange(Q))[None, :] + 0.05 * rng.standard_normal((y.size, Q)))


def time_columns_device(m, Xt, Q, reps):
    ctx = m.ctx
    family, coef, group, G, plain, prior = dmodel._aggregation_spec(m)
    kid = prior.kernelid if prior else 0
    dsm.fit_targets(m, columns(m.y, Q, 7 + Q))
    dsm.predict_targets_gradients(m, Xt, aggregate="device")    # every per-entry array is current from here on
    mom, grd, wall = [], [], []
    for it in range(reps + 1):
        t0 = time.perf_counter()
        ctx.aggregate_columns(family, coef, group, G, plain=plain, prior_kernel_id=kid)
        ctx.aggregate_columns_gradients(plain=plain, prior_kernel_id=kid)
        t1 = time.perf_counter()
        if it:
            mom.append(ctx.agg_columns_seconds)
            grd.append(ctx.agg_columns_gradients_seconds)
            wall.append(t1 - t0)
    rt, D = int(ctx.route_total), int(ctx.D)
    nbytes = 8 * rt * ((Q + 1) + (D * Q + D + Q + 1))
    return dict(Q=Q, aggregate_columns=stats(mom), aggregate_columns_gradients=stats(grd), wall_both_calls=stats(wall),
                gathered_bytes=nbytes, gathered_GBps=nbytes / (np.median(mom) + np.median(grd)) * 1e-9)


def time_columns_host(m, Xt, Q, reps):
    ctx = m.ctx
    xt = np.asfortranarray(Xt)
    n_t = xt.shape[0]
    family, coef, group, G, plain, prior = dmodel._aggregation_spec(m)
    dsm.fit_targets(m, columns(m.y, Q, 7 + Q))
    fetch, lists, col_m, col_g = [], [], [], []
    for it in range(reps + 1):
        dsm.predict(m, xt)
        rc = dmodel._routing(m, xt)
        ptr, idx = rc["lptr"], rc["lidx"]
        t0 = time.perf_counter()
        _, var_l = ctx.predict_fetch()
        mu_l = ctx.predict_targets()
        dmu_l = ctx.predict_targets_gradients()
        _, dvar_l = ctx.predict_gradients()
        t1 = time.perf_counter()
        dev = ctx.predict_targets_seconds + ctx.predict_targets_gradients_seconds + ctx.grad_seconds
        ent = [[] for _ in range(n_t)]
        for l in range(len(ptr) - 1):
            for k in range(int(ptr[l]), int(ptr[l + 1])):
                ent[int(idx[k])].append((l, k))
        t2 = time.perf_counter()
        for j in range(min(Q, 4)):
            a = time.perf_counter()
            dmodel._aggregate_host(m, xt, rc, np.ascontiguousarray(mu_l[:, j]), var_l)
            b = time.perf_counter()
            dsm.aggregate_input_gradients(family, np.ascontiguousarray(mu_l[:, j]), var_l, np.ascontiguousarray(dmu_l[:, :, j]), dvar_l,
                                          ent, coef=coef, group=group, G=G, plain=plain)
            c = time.perf_counter()
            if it:
                col_m.append(b - a)
                col_g.append(c - b)
        if it:
            fetch.append(t1 - t0 - dev)
            lists.append(t2 - t1)
    total = float(np.median(fetch) + np.median(lists) + Q * (np.median(col_m) + np.median(col_g)))
    return dict(Q=Q, fetch_entries=stats(fetch), entry_lists=stats(lists), moments_per_column=stats(col_m),
                gradients_per_column=stats(col_g), host_step_Q_columns=total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mode", default="device", choices=["device", "host"])
    ap.add_argument("--models", default="headline,depth4")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_gradients_time.jsonl"))
    args = ap.parse_args()
    if args.lib:
        hipabi.LIB_PATH = os.path.abspath(args.lib)
        if args.mode == "host":     # a library of the parent commit does not export the new symbols, and this mode calls none
            for name in [n for n in hipabi.SIGNATURES if n.startswith(("dsmgp_aggregate_gradients", "dsmgp_aggregate_columns"))]:
                del hipabi.SIGNATURES[name]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    out = open(args.out, "a")
    X, y, Xt = dsm.regression_data(100_000, 8, seed=20204)
    for name in args.models.split(","):
        m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=MODELS[name], kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                           seed=20204, fit_now=False)
        dsm.fit(m)
        dsm.predict(m, Xt)
        rt = int(m.ctx.route_total)
        rec = dict(what="dsmgp_" + name, mode=args.mode, lib=os.path.basename(hipabi.LIB_PATH), device=m.ctx.device_name(), L=m.L,
                   N=100_000, D=8, n_t=int(Xt.shape[0]), route_total=rt, kind="IsoSE")
        if args.mode == "device":
            rec.update(time_device(m, Xt, args.reps))
            rec["gathered_bytes"] = 8 * (2 * 8 + 2) * rt
            rec["gathered_GBps"] = rec["gathered_bytes"] / rec["sums"]["median"] * 1e-9
        else:
            rec.update(time_host(m, Xt, args.reps))
        base = {k: rec[k] for k in ("what", "mode", "lib", "device", "L", "N", "D", "n_t", "route_total", "kind")}
        lines = [rec]
        for Q in QS:
            lines.append(dict(base, columns=(time_columns_device if args.mode == "device" else time_columns_host)(m, Xt, Q, args.reps)))
        for r in lines:
            line = json.dumps(r)
            print(line, flush=True)
            out.write(line + "\n")
        out.flush()
        m.ctx.close()
    out.close()


if __name__ == "__main__":
    main()
