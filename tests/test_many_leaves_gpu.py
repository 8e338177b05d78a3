"""GPU tests of the leaf-count edges: tables of 33,000 and 65,600 leaves (tests/many_leaves_cases.py) through every entry point
whose launches have one grid row per leaf -- csrc/leaf_chunks.hpp cuts them into runs of 32,768 leaves -- and through everything
that sits behind them.

Reference: for the leaves of 1 to 3 rows (all but five or six of a table) the np.longdouble reference of many_leaves_cases,
which tests/test_many_leaves_host.py holds against 50-digit evaluations; the project's tolerances as they stand, once (one side
rounds).  For the 130-, 150- and 300-row leaves the float64 dense helpers at the other suites' tolerances (doubled: both sides
round).  A library that gave leaf l the rows, test rows or target columns of leaf l - 32768 (or l mod 65536) misses these
tolerances on every leaf past the edge by factors of 10 to 10^11 (the host tests print them).

Each test makes one context for its table and closes it.  Every test prints its wall time by stage and the worst
error / tolerance per quantity (DESIGN.md section 5c records them)."""
import ctypes as C
import time

import numpy as np
import pytest

import many_leaves_cases as mc
from deepstructuredmixtures_amd import hipabi

pytestmark = pytest.mark.gpu

CHUNK = mc.CHUNK
HIP_ATTR_MAX_BLOCK_DIM_X, HIP_ATTR_MAX_GRID_DIM_Y = 26, 30      # hipDeviceAttribute_t (hip_runtime_api.h)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


class _Clock:
    def __init__(self, tag):
        self.tag, self.t0, self.laps = tag, time.perf_counter(), []

    def lap(self, name):
        t = time.perf_counter()
        self.laps.append((name, t - self.t0))
        self.t0 = t

    def show(self):
        print(f"\n{self.tag} wall time: " + ", ".join(f"{n} {s:.2f} s" for n, s in self.laps) + f"; total {sum(s for _, s in self.laps):.2f} s")


def _setup(ctx, t, test=False):
    ctx.set_train(t.X, t.y)
    ctx.set_leaves(t.obs_ptr, t.obs_idx, t.kid, t.mean)
    for k in range(int(t.kid.max()) + 1):
        ctx.set_hyper(k, mc.KINDS[k], mc.HYP[k])
    if t.special:
        ctx.set_sharing(t.op, t.src, t.plen)
    if test:
        ctx.set_test(t.Xt, t.route_ptr, t.route_idx)


def _good(t):
    ok = np.ones(t.L, dtype=bool)
    if t.failed is not None:
        ok[t.failed] = False
    return ok


def _report(tag, worst):
    print(f"\n{tag}: worst error / tolerance  " + ", ".join(f"{k} {v[0]:.3g} (leaf {v[1]})" for k, v in sorted(worst.items())))
    bad = {k: v for k, v in worst.items() if not v[0] <= 1.0}
    assert not bad, (tag, bad)


def _check_small(t, ref, tol, tag, **res):
    got = mc.device_view(t, ref, res)
    _report(tag, mc.compare(got, ref, tol))
    return got


def _check_large(t, ctx, res, leaves, tag):
    """The larger leaves against the float64 dense helpers; `res` as for device_view.  Returns the worst error / tolerance."""
    worst = {}

    def see(key, got, want, tol):
        r = float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.asarray(tol)))
        worst[key] = max(worst.get(key, 0.0), r)

    for l in leaves:
        d = mc.large_leaf(t, l)
        a, b = int(t.obs_ptr[l]), int(t.obs_ptr[l + 1])
        see("mll", res["mll"][l], *d["mll"])
        if "alpha" in res:
            _, alpha = ctx.download_factor(l, b - a, factor=False)
            see("alpha", alpha, *d["alpha"])
        if "grad" in res:
            see("grad", res["grad"][l, :d["grad"][0].size], *d["grad"])
        if "loo" in res:
            lm, lv, ll, tm, tv, ts = d["loo"]
            see("loo_mu", res["loo"][0][a:b], lm, tm), see("loo_var", res["loo"][1][a:b], lv, tv), see("loo_lpd", res["loo"][2][l], ll, ts)
        if "kfold" in res:
            km, kv, kl, tm, tv, tl = d["kfold"]
            see("kfold_mu", res["kfold"][0][a:b], km, tm), see("kfold_var", res["kfold"][1][a:b], kv, tv)
            see("kfold_lpd", res["kfold"][2][l], kl, tl)
            assert np.all(res["kfold"][3][l] == 0)
        if "targets_mll" in res:
            Z, tmll, zt, mt = d["targets"]
            see("targets_mll", res["targets_mll"][l], tmll, mt)
            see("targets_z", ctx.targets_fetch(l), Z, zt)
        if "targets_loo" in res:
            tmu, tlpd, ttm, tts = d["targets_loo"]
            see("targets_loo_mu", res["targets_loo"][0][a:b], tmu, ttm), see("targets_loo_lpd", res["targets_loo"][2][l], tlpd, tts)
        if "pred" in res and t.nt[l]:
            e0, e1 = int(t.route_ptr[l]), int(t.route_ptr[l + 1])
            pm, pv, tm, tv = d["pred"]
            see("pred_mu", res["pred"][0][e0:e1], pm, tm), see("pred_var", res["pred"][1][e0:e1], pv, tv)
    print(f"\n{tag}, leaves {list(leaves)} against the dense helpers: worst error / tolerance  " +
          ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
    assert max(worst.values()) <= 1.0, (tag, worst)


def _check_edge_downloads(t, ctx, ref, tol, tag, targets=True):
    """alpha (download_factor) and Z (targets_fetch) of the small leaves next to the edges and of the special ones."""
    where = {int(l): i for i, l in enumerate(ref["leaves"])}
    wa = wz = wf = 0.0
    count = 0
    for l in t.edge_leaves:
        if int(l) not in where:
            continue
        i, n = where[int(l)], int(t.n[l])
        F, alpha = ctx.download_factor(int(l), n)
        wa = max(wa, float(np.max(np.abs(alpha - ref["alpha"][i, :n]).astype(np.float64) / tol["alpha"][i, :n])))
        # the factor.  F F' = K_y within 16 eps max K_y,ii: the Cholesky's backward error gamma_(n+1) |F||F'| with |F||F'|_ij <=
        # sqrt(K_ii K_jj) (Higham, Accuracy and Stability, theorem 10.3: 4 eps at n = 3), a few eps of the kernel value itself
        # (x exp(-x) <= 0.37: the exponent's rounding does not grow), n eps of the product formed here.  And the log-determinant
        # the reference has, at the log marginal's tolerance (it is one of its terms).
        Ky = np.asarray(ref["Ky"][i, :n, :n], dtype=np.float64)
        F = np.tril(F)
        wf = max(wf, float(np.max(np.abs(F @ F.T - Ky)) / (16.0 * np.finfo(np.float64).eps * np.max(np.diag(Ky)))))
        assert abs(np.sum(np.log(np.diag(F))) - float(ref["half_logdet"][i])) <= tol["mll"][i]
        if targets:
            Z = ctx.targets_fetch(int(l))
            wz = max(wz, float(np.max(np.abs(Z - ref["targets_z"][i, :n]).astype(np.float64) / tol["targets_z"][i, :n])))
        count += 1
    print(f"\n{tag}: {count} edge and special leaves, worst error / tolerance  alpha {wa:.3g}, F F' {wf:.3g}" +
          (f", targets_z {wz:.3g}" if targets else ""))
    assert count >= 10 and wa <= 1.0 and wz <= 1.0 and wf <= 1.0


def test_the_devices_grid_limit():
    """hipDeviceAttributeMaxGridDimY as the runtime reports it (printed: DESIGN.md section 5c records it).  No launch in the
    library has a second grid dimension above 32,768 leaves, 65,535 columns / samples / folds or a few dozen blocks."""
    ctx = hipabi.Context(0)
    try:
        fn = ctx.lib.hipDeviceGetAttribute
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int]
        out = {}
        for name, attr in (("block x", HIP_ATTR_MAX_BLOCK_DIM_X), ("grid x", 29), ("grid y", HIP_ATTR_MAX_GRID_DIM_Y), ("grid z", 31)):
            v = C.c_int(0)
            assert fn(C.byref(v), attr, 0) == 0
            out[name] = v.value
        print(f"\n{ctx.device_name()}: max block dim x {out['block x']}, max grid dim x {out['grid x']}, y {out['grid y']}, z {out['grid z']}")
        assert out["block x"] == 1024            # the enumeration is the one this file names
        assert out["grid y"] >= CHUNK
    finally:
        ctx.close()


def _run_all(ctx, t, clock):
    """fit (the test set riding through it), predictions, gradients, LOO, k-fold, targets and their LOO: everything per leaf."""
    res = {}
    res["mll"], res["info"], _ = ctx.fit()
    clock.lap("fit")
    ctx.predict_run()
    res["pred"] = ctx.predict_fetch()
    clock.lap("predict")
    res["grad"] = ctx.gradients(mc.STRIDE)
    clock.lap("gradients")
    res["loo"] = ctx.loo()
    clock.lap("loo")
    res["kfold"] = ctx.kfold(t.fold, mc.KFOLDS)
    clock.lap("kfold")
    res["targets_mll"], _ = ctx.solve_targets(t.Y, t.Ymean)
    clock.lap("solve_targets")
    res["targets_loo"] = ctx.loo_targets()
    clock.lap("loo_targets")
    return res


def _flat(res):
    out = []
    for k in ("mll", "pred", "grad", "loo", "kfold", "targets_mll", "targets_loo"):
        v = res[k]
        out += [a for a in (v if isinstance(v, tuple) else (v,)) if a is not None and np.asarray(a).dtype == np.float64]
    return out


def test_table_A_every_leaf_against_the_reference():
    """33,000 leaves, one chunk edge, a COPY and a PREFIX leaf across it and a failed leaf past it: fit, the prediction both ways,
    gradients, LOO, k-fold, the target columns and their LOO on every leaf; alpha and Z of the edge leaves."""
    t = mc.table("A")
    clock = _Clock("table A")
    ref = mc.reference(t)
    tol = mc.tolerances(t, ref)
    clock.lap("reference")
    ok, f = _good(t), t.failed
    ctx = hipabi.Context(0)
    try:
        # the standalone sweep: a fit without the test set, then the registration and the prediction
        _setup(ctx, t)
        mll0, info0, _ = ctx.fit()
        ctx.set_test(t.Xt, t.route_ptr, t.route_idx)
        ctx.predict_run()
        alone = ctx.predict_fetch()
        clock.lap("setup, fit, standalone prediction")
        assert np.all(info0[ok] == 0) and info0[f] != 0
        _check_small(t, ref, tol, "table A, standalone prediction", mll=mll0, pred=alone)
        # everything, the test rows riding through the fit
        res = _run_all(ctx, t, clock)
        needed, free = ctx.memory()
        print(f"\ntable A: dsmgp_memory needed {needed / 2**30:.2f} GiB ({needed} bytes), free {free / 2**30:.1f} GiB, lanes {ctx.lanes()}")
        # the COPY claim is kept: the plan holds no factor and no Dinv for leaf 32,770 (to the byte; 2 x 128 x 128 doubles more
        # without it).  The PREFIX claim changes no size; the plan drops one only where it copies no whole block, and this one
        # copies one (tests/test_many_leaves_host.py: plen // 128 == 1)
        assert needed == mc.plan_bytes(t) and t.op[mc.COPY_LEAF] == mc.COPY
        assert np.array_equal(res["info"], info0)
        assert np.all(res["kfold"][3][ok] == 0)
        _check_small(t, ref, tol, "table A, every small leaf", **res)
        clock.lap("compare")
        _check_large(t, ctx, dict(res, alpha=True), t.large, "table A")
        _check_edge_downloads(t, ctx, ref, tol, "table A")
        clock.lap("larger and edge leaves")
        # the failed leaf: NaN where the entry points say so; its neighbours were within tolerance above (leaves f - 1, f + 1)
        a, b = int(t.obs_ptr[f]), int(t.obs_ptr[f + 1])
        e0, e1 = int(t.route_ptr[f]), int(t.route_ptr[f + 1])
        assert np.all(np.isnan(res["loo"][0][a:b])) and np.all(np.isnan(res["loo"][1][a:b])) and np.isnan(res["loo"][2][f])
        assert np.all(np.isnan(res["kfold"][0][a:b])) and np.all(np.isnan(res["kfold"][1][a:b]))
        assert np.all(np.isnan(res["kfold"][2][f])) and np.all(res["kfold"][3][f] == -1)
        assert np.all(np.isnan(res["targets_mll"][f]))
        assert np.all(np.isnan(res["targets_loo"][0][a:b])) and np.all(np.isnan(res["targets_loo"][1][a:b]))
        assert np.all(np.isnan(res["targets_loo"][2][f]))
        print(f"failed leaf {f}: info {info0[f]}, mll {res['mll'][f]}, gradient row {res['grad'][f]}, prediction {res['pred'][0][e0:e1]}")
        for q in (f - 1, f + 1):
            assert t.n[q] <= 3 and info0[q] == 0 and np.isfinite(res["mll"][q]) and np.all(np.isfinite(res["grad"][q]))
        # sharing across the edge: the COPY leaf has its source's factor to the bit and an alpha of its own
        c, s = mc.COPY_LEAF, mc.COPY_SRC
        Fc, ac = ctx.download_factor(c, int(t.n[c]))
        Fs, as_ = ctx.download_factor(s, int(t.n[s]))
        assert _same_bits(Fc, Fs) and not _same_bits(ac, as_)
        p, ps = mc.PREFIX_LEAF, mc.PREFIX_SRC
        Fp, _ = ctx.download_factor(p, int(t.n[p]))
        Fq, _ = ctx.download_factor(ps, int(t.n[ps]))
        assert _same_bits(np.tril(Fp[:128, :128]), np.tril(Fq[:128, :128]))          # the copied block
    finally:
        ctx.close()
    clock.show()


def test_table_A_lanes_fused_steps_and_graph_replay():
    """Table A under one and two lanes (per-leaf results: the same bits), with the fused steps off (within tolerance of the
    reference) and with the fit replayed as a captured graph (the bits of plain launches)."""
    t = mc.table("A")
    clock = _Clock("table A, settings")
    ref = mc.reference(t)
    tol = mc.tolerances(t, ref)
    ok = _good(t)
    ctx = hipabi.Context(0)
    got = {}
    try:
        for lanes in (1, 2):
            ctx.set_option(hipabi.OPT_LANES, lanes)
            _setup(ctx, t, test=True)
            got[lanes] = _run_all(ctx, t, _Clock(""))
            assert ctx.lanes() == lanes
            clock.lap(f"lanes {lanes}")
        for p, q in zip(_flat(got[1]), _flat(got[2])):
            assert _same_bits(p, q)
        assert np.array_equal(got[1]["info"], got[2]["info"]) and np.array_equal(got[1]["kfold"][3], got[2]["kfold"][3])
        _check_small(t, ref, tol, "table A, one lane", **got[1])
        ctx.set_option(hipabi.OPT_LANES, 0)
        # the fit as a graph: captured by the first fit, replayed by the second
        _setup(ctx, t, test=True)
        plain = ctx.fit()
        ctx.set_option(hipabi.OPT_FIT_GRAPH, 1)
        first = ctx.fit()
        again = ctx.fit()
        ctx.predict_run()
        pred = ctx.predict_fetch()
        ctx.set_option(hipabi.OPT_FIT_GRAPH, 0)
        clock.lap("graph")
        for r in (first, again):
            assert _same_bits(r[0][ok], plain[0][ok]) and np.array_equal(r[1], plain[1])
        _check_small(t, ref, tol, "table A, fit replayed as a graph", mll=again[0], pred=pred)
        # fused steps off
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 0)
        _setup(ctx, t, test=True)
        res = {}
        res["mll"], info, _ = ctx.fit()
        ctx.predict_run()
        res["pred"] = ctx.predict_fetch()
        res["grad"] = ctx.gradients(mc.STRIDE)
        res["loo"] = ctx.loo()
        clock.lap("fused steps off")
        assert np.array_equal(info != 0, ~ok)
        _check_small(t, ref, tol, "table A, fused steps off", **res)
        _check_large(t, ctx, res, t.large, "table A, fused steps off")
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_FIT_GRAPH, 0)
        ctx.set_option(hipabi.OPT_LANES, 0)
        ctx.close()
    clock.show()


def test_table_B_every_leaf_against_the_reference():
    """65,600 leaves: past 32,768, 65,535 and 65,536, the third run of every chunked launch holds 64 leaves.  fit on every leaf,
    alpha of the edge leaves (ensure_alpha's copy with L > 65,536), the standalone prediction, the target columns.  No
    gradient, LOO or k-fold pass: L^-T of this table would be another 8.6 GB."""
    t = mc.table("B")
    clock = _Clock("table B")
    ref = mc.reference(t)
    tol = mc.tolerances(t, ref)
    clock.lap("reference")
    ctx = hipabi.Context(0)
    try:
        _setup(ctx, t)
        mll, info, _ = ctx.fit()
        clock.lap("setup, fit")
        needed, free = ctx.memory()
        print(f"\ntable B: dsmgp_memory needed {needed / 2**30:.2f} GiB ({needed} bytes), free {free / 2**30:.1f} GiB, lanes {ctx.lanes()}")
        assert needed == mc.plan_bytes(t)
        assert np.all(info == 0)
        ctx.set_test(t.Xt, t.route_ptr, t.route_idx)
        ctx.predict_run()
        pred = ctx.predict_fetch()
        clock.lap("standalone prediction")
        tmll, _ = ctx.solve_targets(t.Y, t.Ymean)
        clock.lap("solve_targets")
        res = dict(mll=mll, pred=pred, targets_mll=tmll)
        _check_small(t, ref, tol, "table B, every small leaf", **res)
        clock.lap("compare")
        _check_large(t, ctx, dict(res, alpha=True), t.large, "table B")
        _check_edge_downloads(t, ctx, ref, tol, "table B")
        clock.lap("larger and edge leaves")
        past = ref["leaves"] >= 2 * CHUNK
        assert past.sum() == 63 and np.sum(ref["leaves"][ref["routed"]] >= 2 * CHUNK) >= 30      # (leaf L - 1 is a larger one)
    finally:
        ctx.close()
    clock.show()
