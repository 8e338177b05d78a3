"""The step "add the rows and have mu, var of the resident candidates again", with and without the kept test set, on the headline
model of bench.py (its own test set) and at depth 4, for m = 1, 128, 1000 new rows.  Appends one JSON line per measurement to
profiles/resume_time.jsonl.

    python tools/time_resume.py --parent-lib PARENT_LIBRARY.so [--configs dsmgp_n100k_d8 dsmgp_n100k_d8_depth4] [--out FILE]
    python tools/time_resume.py --sums-only CONFIG M      (one step B and the bytes its sums kernel reads: for a kernel trace)

  (A) append_rows + set_test + predict_run with the PARENT commit's library (OUT=... csrc/build.sh in a checkout of it), in a child
      process of its own, which loads that library instead of the package's
  (B) append_rows(keep_test=True) + predict_run with this one
Before either, the model is fitted, the candidates are registered and swept (predict_run).  A and B alternate, three rounds, a
fresh context per measurement (an append cannot be repeated on the same state); the best of the three is kept.  Per step: the
device seconds of its calls, summed (set_test reports none: its device part shows in the wall clock only), and the host wall
clock around the calls (predict_run ends in a synchronise).  Per (config, m) also dsmgp_resume_stats and the bytes of K_tn L^-T
kept, relocated and swept."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M_NEW = (1, 128, 1000)
ROUNDS = 3
TB = 128


class Bench:
    """One model of bench.py on the host; every measurement gets a fresh context, fit, registered and swept candidates."""

    def __init__(self, cfg):
        import bench
        self.cfg = cfg
        self.model, _, _, self.Xt, self.ptr, self.idx = bench.build_model(cfg, 0, 1, 0)
        self.first = True

    def fresh(self):
        import deepstructuredmixtures_amd as dsm
        m = self.model
        if not self.first:
            m.ctx.close()
            m._ctx = None           # (the model makes a new context on first use)
            m._uploaded, m._schedule, m._route_cache = False, None, None
        self.first = False
        dsm.fit(m)
        m.ctx.set_test(self.Xt, self.ptr, self.idx)
        m.ctx.predict_run()
        return m.ctx

    def additions(self, m_new):
        import deepstructuredmixtures_amd as dsm
        from deepstructuredmixtures_amd import tree as ptree
        xn, yn = dsm.regression_data(m_new, self.model.x.shape[1], n_test=1, seed=4000 + m_new)[:2]
        ptr, idx = ptree.route(self.model.root, xn)
        return xn, yn, ptr, idx

    def vt_bytes(self, add_ptr):
        """(kept, swept, read) bytes of K_tn L^-T -- kept and swept as stored (padded rows included); read: what kept_sums_kernel
        loads, the routed rows of every kept real column (a lane loads two rows) -- by the rule of the header: floor(n_old / 128)
        block columns of a leaf that receives rows, every block of one that receives none (no leaf of these models is a failed
        owner; a COPY leaf reads its source's blocks, which have its sizes)."""
        kept = swept = read = 0
        for l, lf in enumerate(self.model.leaves):
            nt = int(self.ptr[l + 1] - self.ptr[l])
            if nt == 0:
                continue
            ntpad = -(-nt // TB) * TB
            add = int(add_ptr[l + 1] - add_ptr[l])
            keep = -(-lf.nobs // TB) if add == 0 else lf.nobs // TB
            kept += ntpad * TB * keep * 8
            swept += ntpad * TB * (-(-(lf.nobs + add) // TB) - keep) * 8
            read += (nt + nt % 2) * min(keep * TB, lf.nobs) * 8
        return kept, swept, read


def step(ctx, b, add, keep_test):
    xn, yn, ptr, idx = add
    t0 = time.perf_counter()
    if keep_test:
        sec = ctx.append_rows(xn, yn, ptr, idx, keep_test=True)[2]
    else:
        sec = ctx.append_rows(xn, yn, ptr, idx)[2]
        ctx.set_test(b.Xt, b.ptr, b.idx)
    sec += ctx.predict_run()
    return dict(device_seconds=sec, wall_seconds=time.perf_counter() - t0)


def serve(lib, cfgs):
    """Child process: the (A) steps with another build of the library, one measurement per line read from stdin."""
    from deepstructuredmixtures_amd import hipabi
    hipabi.LIB_PATH = os.path.abspath(lib)
    for name in ("dsmgp_add_rows_keep_test", "dsmgp_resume_stats", "dsmgp_download_vt"):
        hipabi.SIGNATURES.pop(name, None)
    benches = {}
    for ln in sys.stdin:
        cfg, m = ln.split()
        if cfg not in benches:
            benches[cfg] = Bench(cfg)
        b = benches[cfg]
        print(json.dumps(step(b.fresh(), b, b.additions(int(m)), False)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--configs", nargs="+", default=["dsmgp_n100k_d8", "dsmgp_n100k_d8_depth4"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resume_time.jsonl"))
    ap.add_argument("--sums-only", nargs=2, metavar=("CONFIG", "M"), default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        serve(a.parent_lib, a.configs)
        return
    if a.sums_only:
        b = Bench(a.sums_only[0])
        add = b.additions(int(a.sums_only[1]))
        ctx = b.fresh()
        r = step(ctx, b, add, True)
        print(json.dumps(dict(what="sums_only", config=b.cfg, m=int(a.sums_only[1]), vt_bytes_kept=b.vt_bytes(add[2])[0],
                              sums_kernel_bytes_read=b.vt_bytes(add[2])[2],
                              resume_stats=ctx.resume_stats(), **r)), flush=True)
        ctx.close()
        return
    child = None
    if a.parent_lib:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--parent-lib", a.parent_lib],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    rows = []
    for cfg in a.configs:
        b = Bench(cfg)
        for m in M_NEW:
            add = b.additions(m)
            A, B, stats = [], [], None
            for _ in range(ROUNDS):
                if child:
                    child.stdin.write(f"{cfg} {m}\n")
                    child.stdin.flush()
                    ln = child.stdout.readline()
                    while ln and not ln.startswith("{"):
                        ln = child.stdout.readline()
                    if not ln:
                        raise RuntimeError("the process with the parent library ended early")
                    A.append(json.loads(ln))
                ctx = b.fresh()
                B.append(step(ctx, b, add, True))
                stats = ctx.resume_stats()
            kept, swept, _ = b.vt_bytes(add[2])
            best = lambda runs, k: min(r[k] for r in runs) if runs else None       # noqa: E731
            row = dict(what="resume", config=cfg, leaves=b.model.L, m=m, n_test=int(b.Xt.shape[0]), routed_rows=int(b.ptr[-1]),
                       A_parent_append_set_test_predict=dict(device_seconds=best(A, "device_seconds"), wall_seconds=best(A, "wall_seconds"), runs=A),
                       B_keep_test_predict=dict(device_seconds=best(B, "device_seconds"), wall_seconds=best(B, "wall_seconds"), runs=B),
                       resume_stats=stats, vt_bytes_kept=kept, vt_bytes_relocated=stats["bytes_relocated"], vt_bytes_swept=swept,
                       device=b.model.ctx.device_name().strip())
            if A:
                row["wall_A_over_B"] = best(A, "wall_seconds") / best(B, "wall_seconds")
                row["device_A_over_B"] = best(A, "device_seconds") / best(B, "device_seconds")
            print(json.dumps(row), flush=True)
            rows.append(row)
        b.model.ctx.close()
    if child:
        child.stdin.close()
        child.wait()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
