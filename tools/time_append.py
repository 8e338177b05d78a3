"""dsmgp_append_rows against a refit of the grown table, on the headline model of bench.py and at depth 4, for m = 1, 128, 1000
new rows; and the relocation kernel against plain copies.  Appends one JSON line per measurement to profiles/append_time.jsonl.

    python tools/time_append.py [--yardstick-lib OTHER_LIBRARY.so] [--configs dsmgp_n100k_d8 dsmgp_n100k_d8_depth4] [--out FILE]

Per (config, m): the device seconds of the call (ONE call, the first on its context: an append cannot be repeated on the same
state; the refit beside it is the best of three), what dsmgp_append_stats says it did, the algorithmic flops of its update and
fused launches (dsmgp_work, dsmgp_work_fused), and the device seconds and flops of a from-scratch dsmgp_fit of the same grown
table -- with THIS library or, given --yardstick-lib, with that build (the parent commit's: the yardstick the call is judged by;
it runs in a child process of its own, which loads that library instead of the package's).
The relocation kernel (needs the diagnostic build, csrc/build.sh diag): bytes per second of the one launch beside one contiguous
device-to-device hipMemcpy of the same byte count and beside the hipMemcpy2DAsync + hipMemcpyAsync pair per leaf that the PREFIX
phase of dsmgp_fit issues, at the leaf count and block sizes of the depth-4 model."""
import argparse
import json
import os
import subprocess
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M_NEW = (1, 128, 1000)


def _fitted_model(cfg):
    import bench
    import deepstructuredmixtures_amd as dsm
    model = bench.build_model(cfg, 0, 1, 0)[0]
    dsm.fit(model)
    return model


def _new_rows(model, m):
    import deepstructuredmixtures_amd as dsm
    return dsm.regression_data(m, model.x.shape[1], n_test=1, seed=4000 + m)[:2]


def _refit_seconds(cfg, m):
    """Device seconds and update flops of dsmgp_fit from scratch on the grown table: add_data's own out-of-memory fallback, taken
    on purpose (the context's append_rows is replaced by one that reports DSMGP_E_NOMEM)."""
    import deepstructuredmixtures_amd as dsm
    from deepstructuredmixtures_amd import hipabi
    model = _fitted_model(cfg)

    def no_room(*a, **k):
        raise hipabi.DsmgpError(hipabi.E_NOMEM, "time_append: the refit is what is being timed")
    model.ctx.append_rows = no_room
    xn, yn = _new_rows(model, m)
    sec = dsm.add_data(model, xn, yn)
    assert sec.fallback
    best = float(sec)
    for _ in range(2):                      # the table is resident now: plain refits, best of three
        best = min(best, float(dsm.fit(model)))
    out = dict(refit_seconds=best, refit_update_flops=model.ctx.work()[0], refit_fused_flops=model.ctx.work_fused()[0])
    model.ctx.close()
    return out


def yardstick(lib, cfgs):
    """Child process: the refits with another build of the library (it has no dsmgp_append_rows: the binding is told so)."""
    from deepstructuredmixtures_amd import hipabi
    hipabi.LIB_PATH = os.path.abspath(lib)
    for name in ("dsmgp_append_rows", "dsmgp_append_stats"):
        hipabi.SIGNATURES.pop(name, None)
    for cfg in cfgs:
        for m in M_NEW:
            print(json.dumps(dict(config=cfg, m=m, **_refit_seconds(cfg, m))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--yardstick-lib", default=None)
    ap.add_argument("--configs", nargs="+", default=["dsmgp_n100k_d8", "dsmgp_n100k_d8_depth4"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_time.jsonl"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        yardstick(a.yardstick_lib, a.configs)
        return
    import deepstructuredmixtures_amd as dsm
    from deepstructuredmixtures_amd import hipabi
    parent = {}
    if a.yardstick_lib:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--yardstick-lib", a.yardstick_lib, "--configs"] + a.configs,
                           capture_output=True, text=True, check=True, cwd=ROOT)
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                d = json.loads(ln)
                parent[(d["config"], d["m"])] = d
    rows = []
    for cfg in a.configs:
        for m in M_NEW:
            model = _fitted_model(cfg)
            full = dict(fit_seconds=float(model.last_fit_seconds), fit_update_flops=model.ctx.work()[0], fit_fused_flops=model.ctx.work_fused()[0])
            xn, yn = _new_rows(model, m)
            sec = dsm.add_data(model, xn, yn)
            row = dict(what="append_rows", config=cfg, leaves=model.L, m=m, append_seconds=float(sec), fallback=bool(sec.fallback),
                       stats=sec.stats, path="in place" if sec.stats and sec.stats["bytes_relocated"] == 0 else "relocate",
                       append_update_flops=model.ctx.work()[0], append_fused_flops=model.ctx.work_fused()[0],
                       fit_before=full, device=model.ctx.device_name().strip())
            model.ctx.close()
            if (cfg, m) not in parent:
                row["refit_this_library"] = _refit_seconds(cfg, m)
            else:
                p = parent[(cfg, m)]
                row["refit_yardstick_library"] = {k: p[k] for k in ("refit_seconds", "refit_update_flops", "refit_fused_flops")}
                row["speedup_over_yardstick_refit"] = p["refit_seconds"] / float(sec)
            print(json.dumps(row), flush=True)
            rows.append(row)
    # the relocation kernel at the shape of the depth-4 model: 18,461 leaves, factors of 1..20 blocks; here every leaf keeps
    # kb blocks and grows by one block row (ld_new = ld_old + 128)
    if os.path.exists(hipabi.DIAG_LIB_PATH):
        c = hipabi.Context(0, diag=True)
        for nleaves, kb in ((18461, 1), (8192, 2), (4096, 4), (64, 32)):
            r = c.bench_relocate(nleaves, kb, kb * 128, (kb + 1) * 128, reps=5)
            row = dict(what="relocate_tiles_kernel", leaves=nleaves, kept_blocks=kb, bytes=r["bytes"],
                       kernel_seconds=r["kernel_s"], memcpy_seconds=r["memcpy_s"], per_leaf_copies_seconds=r["per_leaf_copies_s"],
                       kernel_GBps=r["bytes"] / r["kernel_s"] / 1e9, memcpy_GBps=r["bytes"] / r["memcpy_s"] / 1e9,
                       per_leaf_copies_GBps=r["bytes"] / r["per_leaf_copies_s"] / 1e9, device=c.device_name().strip())
            print(json.dumps(row), flush=True)
            rows.append(row)
        c.close()
    else:
        print("no diagnostic build: the relocation kernel is not timed", file=sys.stderr)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
