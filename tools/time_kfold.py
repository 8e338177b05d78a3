"""Device time of dsmgp_kfold beside what it replaces, one JSON line per cell (profiles/kfold_time.jsonl):
  the headline model (N = 100k, D = 8, depth 2) at K = 5 and 10, depth 4 at K = 5, a single GP n = 4096 at K = 5, 10, 64,
  random balanced labels (make_folds).
`kfold_fresh` = kfold() right after a fit (the call inverts L^-T), `kfold_current` = kfold() again on the same fit (reads it),
each with its four-way split (L^-T, pack + G_FF, factorisation, inverse factors + moments); `refits` = the device seconds of K
rounds of set_leaves (every leaf without the fold's rows, every leaf factorised in full: no sharing schedule), fit, set_test on the
held-out rows of every leaf and predict_run.  Medians of `--reps` repetitions.  With --refits-only the script needs nothing of
dsmgp_kfold and runs against an older library as well (the labels then come from the same counter stream, inlined below);
--merge-parent FILE takes the `refits` of such a run's output, cell by cell, into the column `refits_parent_library`.
profiles/kfold_time.jsonl is the output of
    (in a checkout of the parent commit, this script copied in)  python tools/time_kfold.py --refits-only > parent.jsonl
    python tools/time_kfold.py --merge-parent parent.jsonl
Usage:  python tools/time_kfold.py [--reps 3] [--cells headline5,headline10,depth4,gp5,gp10,gp64] [--refits-only]
                                   [--merge-parent FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deepstructuredmixtures_amd as dsm  # noqa: E402
from deepstructuredmixtures_amd import datagen, hipabi  # noqa: E402
from deepstructuredmixtures_amd.tree import obs_table  # noqa: E402


PARENT = {}     # cell -> refits of a --refits-only run on the parent commit (--merge-parent)


def folds(n, K, seed=0):
    """make_folds(n, K, seed) without groups (kept here so that the script runs on a tree that has no make_folds)."""
    order = np.argsort(datagen.uniform(int(seed), 0, n), kind="stable")
    label = np.empty(n, dtype=np.int32)
    label[order] = (np.arange(n) % K).astype(np.int32)
    return label


def med(a):
    return float(np.median(np.asarray(a, dtype=np.float64)))


def refit_rounds(ctx, X, ptr, idx, kid, mean, fold, K):
    """Device seconds of the K rounds, and the held-out means of the last one (so that the work is not optimised away)."""
    L = len(ptr) - 1
    total = 0.0
    for k in range(K):
        keep = fold[idx] != k
        nptr = np.concatenate([[0], np.cumsum([int(np.sum(keep[ptr[l]:ptr[l + 1]])) for l in range(L)])]).astype(np.int64)
        ctx.set_leaves(nptr, idx[keep], kid, mean)
        rows = np.flatnonzero(fold == k)
        where = np.full(fold.size, -1, dtype=np.int64)
        where[rows] = np.arange(rows.size)
        held = ~keep
        rptr = np.concatenate([[0], np.cumsum([int(np.sum(held[ptr[l]:ptr[l + 1]])) for l in range(L)])]).astype(np.int64)
        ctx.set_test(np.asfortranarray(X[rows]), rptr, where[idx[held]])
        _, info, sec = ctx.fit()
        assert np.all(info == 0)
        total += sec + ctx.predict_run()
    ctx.predict_fetch()
    return total


def cell(name, ctx, X, ptr, idx, kid, mean, K, reps, refits_only, restore, extra):
    fold = folds(X.shape[0], K, seed=K)
    out = dict(cell=name, K=K, **extra)
    if not refits_only:
        fresh, cur, sf, sc = [], [], [], []
        for _ in range(reps):
            restore()
            ctx.fit()
            ctx.kfold(fold, K)
            fresh.append(ctx.kfold_seconds)
            sf.append(ctx.kfold_split_seconds.copy())
            ctx.kfold(fold, K)
            cur.append(ctx.kfold_seconds)
            sc.append(ctx.kfold_split_seconds.copy())
        out.update(kfold_fresh=med(fresh), kfold_fresh_split=[float(v) for v in np.median(sf, axis=0)],
                   kfold_current=med(cur), kfold_current_split=[float(v) for v in np.median(sc, axis=0)])
    out["refits"] = med([refit_rounds(ctx, X, ptr, idx, kid, mean, fold, K) for _ in range(reps)])
    if name in PARENT:
        out["refits_parent_library"] = PARENT[name]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cells", default="headline5,headline10,depth4,gp5,gp10,gp64")
    ap.add_argument("--refits-only", action="store_true")
    ap.add_argument("--merge-parent", default=None)
    args = ap.parse_args()
    if args.merge_parent:
        for line in open(args.merge_parent):
            d = json.loads(line)
            if "cell" in d:
                PARENT[d["cell"]] = d["refits"]
    cells = args.cells.split(",")
    gp = [c for c in cells if c.startswith("gp")]
    if gp:
        n, D = 4096, 4
        X, y, _ = dsm.regression_data(n, D, n_test=8, seed=20202)
        ctx = hipabi.Context(0)
        ctx.set_train(X, y)
        ptr, idx, kid, mean = np.array([0, n], dtype=np.int64), np.arange(n, dtype=np.int64), [0], [float(np.mean(y))]
        ctx.set_hyper(0, 0, np.array([np.log(0.5), 0.0, np.log(0.1)]))
        print(json.dumps(dict(device=ctx.device_name(), refits_only=args.refits_only)), flush=True)
        for c in gp:
            cell(c, ctx, X, ptr, idx, kid, mean, int(c[2:]), args.reps, args.refits_only,
                 lambda: ctx.set_leaves(ptr, idx, kid, mean), dict(n=n, D=D, L=1))
        ctx.close()
    for name, depth, Ks in (("headline", 2, [int(c[8:]) for c in cells if c.startswith("headline")]),
                            ("depth4", 4, [5] if "depth4" in cells else [])):
        if not Ks:
            continue
        X, y, _ = dsm.regression_data(100_000, 8, seed=20204)
        m = dsm.buildDSMGP(X, y, 3, 4, M=200, D=depth, kernel=dsm.IsoSE(float(np.log(0.3)), 0.0), logNoise=float(np.log(0.1)),
                           seed=20204, fit_now=False)
        dsm.fit(m)
        ptr, idx = obs_table(m.leaves)
        ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
        kid, mean = [lf.kernelid for lf in m.leaves], [lf.mean.m for lf in m.leaves]

        def restore():
            m._uploaded = False
            dsm.fit(m)

        for K in Ks:
            cell(f"{name}{K}" if name == "headline" else name, m.ctx, X, ptr, idx, kid, mean, K, args.reps, args.refits_only, restore,
                 dict(N=100_000, D=8, L=m.L))
        m.ctx.close()


if __name__ == "__main__":
    main()
