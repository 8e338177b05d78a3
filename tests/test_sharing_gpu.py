"""GPU tests of the shared-Cholesky schedule: the tables of tests/sharing_tables.py (every PREFIX geometry at a block edge, both
phases under both step kinds) in every schedule cell, against the 50-digit fixture tests/golden/gp_sharing.npz (sets of at most
512 rows), the float64 oracle (larger sets) and the unshared fit of the same cell.  No tolerance here is new: each is the
function or constant the suite already uses for the same quantity, named where it is used."""
import itertools

import numpy as np
import pytest

import scipy.linalg as sla

import dense_gp
import dense_kernels as dk
import loo_dense
import loo_grad_dense as lgd
import predgrad_dense as pgd
import sharing_tables as st
import targets_dense as td
import targets_grad_dense as tgd
from deepstructuredmixtures_amd import hipabi
from pred_tolerance import alpha_tol, mll_tol, moment_tol
from test_predcov_gpu import entry_tol

pytestmark = pytest.mark.gpu

RTOL = 1e-8       # tests/test_gpu_parity.py: the oracle comparison of test_fused_tile_tasks_pack_ragged_row_blocks
DEFAULTS = dict(fused_steps=1, diag_in_update=1, lanes=1, joint=True, fused_gram=1, graph=0)
OPTION_OF = dict(fused_steps=hipabi.OPT_FUSED_STEPS, diag_in_update=hipabi.OPT_DIAG_IN_UPDATE, lanes=hipabi.OPT_LANES,
                 fused_gram=hipabi.OPT_FUSED_GRAM, graph=hipabi.OPT_FIT_GRAPH)
RESTORE = dict(fused_steps=1, diag_in_update=1, lanes=0, fused_gram=1, graph=0)        # the library's defaults


def _cell_id(c):
    return (f"steps{c['fused_steps']}-ahead{c['diag_in_update']}-lanes{c['lanes']}-{'joint' if c['joint'] else 'standalone'}"
            + ("" if c["fused_gram"] else "-gramlaunch") + ("-graph" if c["graph"] else ""))


CELLS = [dict(DEFAULTS, fused_steps=a, diag_in_update=b, lanes=c, joint=d)
         for a, b, c, d in itertools.product((1, 0), (1, 0), (1, 2), (True, False))]
CELLS += [dict(DEFAULTS, fused_gram=0), dict(DEFAULTS, graph=1)]
WIDE_CELLS = [dict(DEFAULTS, lanes=c, joint=d) for c, d in itertools.product((1, 2), (True, False))]   # D = 33: no fused Gram
CORE = [(t, c) for t in ("T1", "T2", "T3", "T4") for c in CELLS] + [("T4d33", c) for c in WIDE_CELLS]


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return st.load_golden()


_TABLES, _ORACLE = {}, {}


def _table(name):
    if name not in _TABLES:
        _TABLES[name] = st.table(name)
    return _TABLES[name]


def _oracle(t, l):
    """(mll, mu, var) of the float64 oracle leaf, computed once per set."""
    key = (t.D, t.keys[l])
    if key not in _ORACLE:
        g = t.oracle(l)
        assert g.info == 0
        mu, var = g.prediction(t.Xt[t.routes[l]]) if t.routes[l].size else (np.zeros(0), np.zeros(0))
        _ORACLE[key] = (g.mll(), mu, var)
    return _ORACLE[key]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class _Options:
    """Sets the cell's options and restores the library's defaults on the way out."""

    def __init__(self, ctx, cell):
        self.ctx, self.cell = ctx, cell

    def __enter__(self):
        for k, opt in OPTION_OF.items():
            self.ctx.set_option(opt, self.cell[k])
        self.ctx.set_profile(0)
        return self

    def __exit__(self, *exc):
        for k, opt in OPTION_OF.items():
            self.ctx.set_option(opt, RESTORE[k])
        self.ctx.set_joint(True)
        return False


def _run(ctx, t, cell, sharing=True, leaves=None, schedule=None, references=True):
    """One fit and prediction of table `t` under the options in force: mll, info, mu, var, (F, alpha) of `leaves`, the number of
    fused tile launches of the fit, the lanes of the plan."""
    t.load(ctx, sharing)
    if schedule is not None:
        ctx.set_sharing(*schedule)
    if cell["joint"]:
        ctx.set_test(t.Xt, t.route_ptr, t.route_idx)        # the rows ride through the factorisation launches
    mll, info, _ = ctx.fit()
    fused = ctx.work_fused()[1]
    if not cell["joint"]:
        ctx.set_test(t.Xt, t.route_ptr, t.route_idx)        # registered after the fit: the standalone sweep
    ctx.predict_run()
    mu, var = ctx.predict_fetch()
    fa = {l: ctx.download_factor(l, int(t.n[l])) for l in (t.shared() if leaves is None else leaves)}
    alpha = {l: fa[l][1] if l in fa else ctx.download_factor(l, int(t.n[l]), factor=False)[1]
             for l in range(t.L) if l in fa or (references and t.n[l] <= st.MAX_MP_ROWS)}
    return dict(mll=mll, info=info, mu=mu, var=var, fa=fa, alpha=alpha, fused=fused, lanes=ctx.lanes())


def _check_references(t, res, golden):
    """Every leaf against the 50 digits (pred_tolerance.mll_tol / alpha_tol / moment_tol) where its set has an entry, else
    against the float64 oracle at the tolerances of test_fused_tile_tasks_pack_ragged_row_blocks.  Returns the worst
    error / tolerance of either kind."""
    assert np.all(res["info"] == 0), np.flatnonzero(res["info"])
    worst_mp = worst_o = 0.0
    for l in range(t.L):
        a, b = int(t.route_ptr[l]), int(t.route_ptr[l + 1])
        mu, var = res["mu"][a:b], res["var"][a:b]
        g = golden.get(t.keys[l]) if t.D == 3 else None
        if g is not None:
            o = t.obs[l]
            alpha = res["alpha"][l]
            noise = float(np.exp(2.0 * t.hyp(l)[-1]))
            tm, tv = moment_tol(g["mu"], g["var"], g["kss"], noise, max(1.0, float(np.max(np.abs(t.y[o])))))
            r = [abs(res["mll"][l] - g["mll"]) / float(mll_tol(g["mll"], g["cond"])),
                 float(np.max(np.abs(alpha - g["alpha"]))) / alpha_tol(g["alpha"], g["cond"])]
            if b > a:
                r += [float(np.max(np.abs(mu - g["mu"]) / tm)), float(np.max(np.abs(var - g["var"]) / tv))]
            assert max(r) <= 1.0, (t.name, l, t.keys[l], r)
            worst_mp = max(worst_mp, max(r))
        else:
            m_o, mu_o, var_o = _oracle(t, l)
            r = [abs(res["mll"][l] - m_o) / (RTOL * abs(m_o))]
            if b > a:
                r += [float(np.max(np.abs(mu - mu_o) / (1e-9 + RTOL * np.abs(mu_o)))),
                      float(np.max(np.abs(var - var_o) / (1e-10 + RTOL * np.abs(var_o))))]
            assert max(r) <= 1.0, (t.name, l, t.keys[l], r)
            worst_o = max(worst_o, max(r))
    return worst_mp, worst_o


def _check_cross(t, shared, plain, leaves=None):
    """The shared leaves against the unshared fit of the same cell, at the bounds of
    test_prefix_continue_equals_full_factorisation: factor 1e-12 max|F|, mll rtol 1e-12, alpha rtol 1e-9 and atol 1e-11 -- the
    absolute term per unit of alpha's own scale max(1, max|alpha|), as pred_tolerance.ATOL is defined: that test's alpha is of
    order 1..10, an ArdLinear leaf's here reaches 77 next to entries of 0.002, and two correct solves differ by a multiple of
    cond_2(K_y) eps max|alpha| (4.7e4 x 1.1e-16 x 77 = 4e-10 for the 639-row leaf g128_129/big6, whose two alphas are 1.4e-11
    apart in the fused cells: 1.2 times the unscaled term, while each is within 0.002 pred_tolerance.alpha_tol of the 50-digit
    alpha -- DESIGN.md section 5a).  Returns the worst error / bound."""
    worst = 0.0
    for l in (t.shared() if leaves is None else leaves):
        (Fs, as_), (Ff, af) = shared["fa"][l], plain["fa"][l]
        scale = max(1.0, float(np.max(np.abs(af))))
        r = [float(np.max(np.abs(Fs - Ff))) / (1e-12 * float(np.max(np.abs(Ff)))),
             abs(shared["mll"][l] - plain["mll"][l]) / (1e-12 * abs(plain["mll"][l])),
             float(np.max(np.abs(as_ - af) / (1e-11 * scale + 1e-9 * np.abs(af))))]
        assert max(r) <= 1.0, (t.name, l, t.keys[l], int(t.n[l]), r)
        worst = max(worst, max(r))
    return worst


# ------------------------------------------------------------------------------------- (a) every table in every schedule cell

@pytest.mark.parametrize("name,cell", CORE, ids=[f"{n}-{_cell_id(c)}" for n, c in CORE])
def test_table_in_schedule_cell(ctx, golden, name, cell):
    """Shared fit and prediction of one table under one combination of step kinds, lookahead, lanes, route to K_tn L^-T, Gram
    launch and graph replay: every leaf against its reference, every PREFIX and COPY leaf's factor, log-marginal and alpha
    against the unshared fit under the same options."""
    t = _table(name)
    with _Options(ctx, cell):
        shared = _run(ctx, t, cell)
        assert shared["lanes"] == cell["lanes"]
        if cell["graph"]:                  # the replayed fit: the bits of plain launches under the same options
            with _Options(ctx, dict(cell, graph=0)):
                launched = _run(ctx, t, cell)
            for k in ("mll", "info", "mu", "var"):
                assert _same_bits(shared[k], launched[k]), k
            for l in t.shared():
                assert _same_bits(shared["fa"][l][0], launched["fa"][l][0]) and _same_bits(shared["fa"][l][1], launched["fa"][l][1])
            for k, opt in OPTION_OF.items():
                ctx.set_option(opt, cell[k])
        worst_mp, worst_o = _check_references(t, shared, golden)
        plain = _run(ctx, t, cell, sharing=False)
        worst_x = _check_cross(t, shared, plain)
    print(f"\n{name} {_cell_id(cell)}: worst error / tolerance: 50 digits {worst_mp:.3g}, oracle {worst_o:.3g}, "
          f"shared against unshared {worst_x:.3g}")


# ------------------------------------------------------------------------------------- (b) the schedule under test really ran

@pytest.mark.parametrize("joint", [True, False], ids=["joint", "standalone"])
def test_fused_launches_belong_to_the_expected_phase(ctx, joint):
    """dsmgp_work_fused counts the fused tile launches of a fit.  The table without its phase-1 leaves (sources, fillers and COPY
    leaves: sharing_tables.Table.reduced) launches those of phase 0 alone, so the difference is phase 1's: more than none in T1
    and T2, none in T3 and T4; phase 0 launches some in T1 and T3 and none in T2 and T4.  One lane: a launch per fused step.
    A plan that quietly ran the steps classic fails here."""
    cell = dict(DEFAULTS, joint=joint)
    count = {}
    with _Options(ctx, cell):
        for name in ("T1", "T2", "T3", "T4"):
            t = _table(name)
            full = _run(ctx, t, cell, leaves=[], references=False)
            part = _run(ctx, t.reduced(), cell, leaves=[], references=False)
            assert np.all(full["info"] == 0) and np.all(part["info"] == 0)
            count[name] = (full["fused"], part["fused"])
    print(f"\nfused tile launches (table, its phase-0 leaves alone): {count}")
    for name in ("T1", "T2", "T3", "T4"):
        t = _table(name)
        full, part = count[name]
        assert (part > 0) == bool(t.fused[0]), (name, count)
        assert (full > part) == bool(t.fused[1]) and full >= part, (name, count)
    assert count["T2"][1] == 0 and count["T2"][0] > 0 and count["T4"] == (0, 0)
    with _Options(ctx, dict(cell, fused_steps=0)):
        assert _run(ctx, _table("T1"), cell, leaves=[], references=False)["fused"] == 0


# ------------------------------------------------------------------------------------- (c) downstream calls on the shared leaves

Q_TARGETS = 3
_DENSE = {}


def _targets(t):
    """Q = 3 target columns over the training rows (column 0 is y), a mean per (leaf, column) -- column 0 the fit's, so a COPY
    leaf with a mean of its own keeps it in every column -- and weights of mixed sign per (leaf, column).  All three are
    functions of the leaf's set."""
    X = t.X
    Y = np.stack([t.y, np.cos(2.0 * X[:, 0]) + X[:, 1], np.sin(4.0 * X[:, 2]) - 0.5 * X[:, 0]], axis=1)
    mean = np.stack([np.mean(Y[o], axis=0) for o in t.obs])
    mean[:, 0] = t.mean
    for l in t.leaves(st.COPY):
        mean[l, 1:] += t.mean[l] - t.mean[t.src[l]]
    order = {k: i for i, k in enumerate(sorted(t.dat.sets))}      # weights by set: tables that share a set share its reference
    W = np.stack([0.25 + 1.5 * st.uniform(7950, order[k] * Q_TARGETS, Q_TARGETS) for k in t.keys])
    W[:, 1] *= -1.0
    W[[l for l, k in enumerate(t.keys) if order[k] % 3 == 1], 2] *= -1.0
    return np.asfortranarray(Y), mean, W


def _dense(t, l, Y, mean, W):
    """The float64 dense restatement of every downstream call for leaf l, from SciPy's factor of K + (noise + 1e-8) I of the
    leaf's own rows, own targets and own mean: computed once per set and shared by the cells."""
    key = (t.D, t.keys[l])
    if key in _DENSE:
        return _DENSE[key]
    kind, hyp = t.kind(l), t.hyp(l)
    h, logNoise = hyp[:-1], float(hyp[-1])
    noise = float(np.exp(2.0 * logNoise))
    o = t.obs[l]
    Xl, yl, Yl, m = np.asfortranarray(t.X[o]), t.y[o], Y[o], float(t.mean[l])
    Xr = np.asfortranarray(t.Xt[t.routes[l]])
    n, D = Xl.shape
    r = {}
    # gradients and the per-column gradients: the textbook trace, tests/targets_grad_dense.py (the library's conventions)
    G, _, cond = tgd.column_gradients(kind, hyp, Xl, Yl, mean[l])
    r["cond"] = cond
    r["grad"] = (G[0], 2.0 * tgd.tolerance(G[:1], [1.0], cond))
    r["tgrad"] = (tgd.weighted(G, W[l]), 2.0 * tgd.tolerance(G, W[l], cond))
    # leave-one-out moments and density: tests/loo_dense.py
    K, dKs = dk.d_hyper(kind, h, Xl)
    lmu, lvar, lpd = loo_dense.loo_dense(K, noise, yl, m)
    tm, tv, _, tsum = loo_dense.loo_tol(yl, lmu, lvar, np.diag(K), noise)
    r["loo"] = (lmu, 2.0 * tm, lvar, 2.0 * tv, float(np.sum(lpd)), 2.0 * tsum)
    # LOO gradients: tests/loo_grad_dense.py on the true kernel derivatives
    lg = lgd.loo_grad_dense(K, dKs, noise, yl, m)
    r["loograd"] = (lg, 2.0 * lgd.tolerance(dict(kind=kind, cond=cond, weak=False, logNoise=logNoise), lg))
    # targets: tests/targets_dense.py on the dense factor
    F = dense_gp.factor(K, noise)
    Ktn = dk.value(kind, h, Xr, Xl) if Xr.shape[0] else None
    Z, tmll, tmu = td.reference(F, Yl, mean[l], Ktn)
    r["targets"] = (Z, 2.0 * td.z_tol(Z, cond), tmll, 2.0 * td.mll_tol(Z, F, cond), tmu,
                    None if tmu is None else 2.0 * td.mu_tol(tmu, Yl))
    if Xr.shape[0]:
        # full predictive covariance: as tests/test_predcov_gpu.py
        V = sla.solve_triangular(F, Ktn.T, lower=True)
        S = dk.value(kind, h, Xr, Xr) - V.T @ V
        kss = st.prior_diag(kind, hyp, Xr)
        r["cov"] = (S, 2.0 * entry_tol(S, kss, noise), noise)
        # input gradients: tests/predgrad_dense.py
        _, _, dmu, dvar = pgd.moments(kind, h, logNoise, Xl, yl, m, Xr)
        tdm, tdv = pgd.tolerances(kind, h, logNoise, Xl, yl, Xr, dmu, dvar)
        r["pgrad"] = (dmu, 2.0 * tdm, dvar, 2.0 * tdv)
    _DENSE[key] = r
    return r


def _ratio(got, ref, tol):
    return float(np.max(np.abs(np.asarray(got) - ref) / tol)) if np.size(ref) else 0.0


def _downstream(ctx, t, Y, mean, W, stride):
    """Every downstream call on the current fit."""
    out = dict(grad=ctx.gradients(stride), loo=ctx.loo(), loograd=ctx.loo_gradients(stride)[0])
    out["pgrad"] = ctx.predict_gradients()
    out["tmll"], _ = ctx.solve_targets(Y, mean)
    out["tmu"] = ctx.predict_targets()
    out["tgrad"] = ctx.targets_gradients(stride, W)
    out["Z"] = {l: ctx.targets_fetch(l) for l in t.shared()}
    out["cov"] = {(l, wn): ctx.predict_cov(l, t.routes[l].size, with_noise=wn) for l in t.shared() if t.routes[l].size
                  for wn in (True, False)}
    return out


def _check_downstream(t, out, Y, mean, W):
    """The shared leaves of one run against their dense leaves; returns the worst error / tolerance per call."""
    worst = {}
    for l in t.shared():
        d = _dense(t, l, Y, mean, W)
        a, b = int(t.obs_ptr[l]), int(t.obs_ptr[l + 1])
        e0, e1 = int(t.route_ptr[l]), int(t.route_ptr[l + 1])
        nh = d["grad"][0].size
        r = dict(gradients=_ratio(out["grad"][l, :nh], *d["grad"]), targets_gradients=_ratio(out["tgrad"][l, :nh], *d["tgrad"]),
                 loo_gradients=_ratio(out["loograd"][l, :nh], *d["loograd"]))
        assert np.all(out["grad"][l, nh:] == 0.0) and np.all(out["tgrad"][l, nh:] == 0.0) and np.all(out["loograd"][l, nh:] == 0.0)
        lmu, tm, lvar, tv, lpd, tsum = d["loo"]
        r["loo"] = max(_ratio(out["loo"][0][a:b], lmu, tm), _ratio(out["loo"][1][a:b], lvar, tv),
                       abs(out["loo"][2][l] - lpd) / tsum)
        Z, tz, tmll, tml, tmu, tmt = d["targets"]
        r["solve_targets"] = max(_ratio(out["Z"][l], Z, tz), _ratio(out["tmll"][l], tmll, tml))
        if e1 > e0:
            r["predict_targets"] = _ratio(out["tmu"][e0:e1], tmu, tmt)
            S, ts, noise = d["cov"]
            for wn in (True, False):
                C = out["cov"][(l, wn)]
                assert _same_bits(C, C.T), (l, wn)                                   # symmetric to the bit
                r["predict_cov"] = max(r.get("predict_cov", 0.0), _ratio(C, S + (noise * np.eye(e1 - e0) if wn else 0.0), ts))
            dmu, tdm, dvar, tdv = d["pgrad"]
            r["predict_gradients"] = max(_ratio(out["pgrad"][0][e0:e1], dmu, tdm), _ratio(out["pgrad"][1][e0:e1], dvar, tdv))
        assert max(r.values()) <= 1.0, (t.name, l, t.keys[l], r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


DOWNSTREAM = [("T1", "defaults", DEFAULTS), ("T1", "classic", dict(DEFAULTS, fused_steps=0, diag_in_update=0)),
              ("T1", "lanes2", dict(DEFAULTS, lanes=2)), ("T2", "defaults", DEFAULTS),
              ("T2", "classic", dict(DEFAULTS, fused_steps=0, diag_in_update=0)), ("T2", "lanes2", dict(DEFAULTS, lanes=2)),
              ("T4", "defaults", DEFAULTS)]


@pytest.mark.parametrize("name,tag,cell", DOWNSTREAM, ids=[f"{n}-{g}" for n, g, _ in DOWNSTREAM])
def test_downstream_calls_on_the_shared_leaves(ctx, name, tag, cell):
    """gradients, loo, loo_gradients, predict_cov (with and without noise, symmetric to the bit), predict_gradients,
    solve_targets (Q = 3, column 0 = y) / predict_targets and targets_gradients (signed weights per leaf and column) for every
    PREFIX and COPY leaf against the float64 dense restatement of its own leaf -- own rows, own targets, own mean: the COPY leaf
    with a mean of its own is not its source -- within twice that module's tolerance (both sides are float64).  The unshared
    fit of the same cell is held to the same references; gradients and targets_gradients also agree across the two fits to
    the relative bounds their sibling tests use across step kinds and contexts (1e-11, 1e-12).  A leaf mask that selects the
    PREFIX leaves gives their unmasked rows and zeros elsewhere."""
    t = _table(name)
    Y, mean, W = _targets(t)
    stride = max(h.size for _, h in t.hyper.values())
    runs = []
    with _Options(ctx, cell):
        for sharing in (True, False):
            res = _run(ctx, t, cell, sharing=sharing, leaves=[], references=False)
            assert np.all(res["info"] == 0) and res["lanes"] == cell["lanes"]
            out = _downstream(ctx, t, Y, mean, W, stride)
            runs.append(out)
            worst = _check_downstream(t, out, Y, mean, W)
            print(f"\n{name} {tag} {'shared' if sharing else 'unshared'}: worst error / tolerance "
                  + ", ".join(f"{k} {v:.3g}" for k, v in sorted(worst.items())))
            if sharing:
                mask = (t.op == st.PREFIX).astype(np.int32)
                ctx.set_gradient_leaves(mask)
                try:
                    masked = ctx.gradients(stride)
                finally:
                    ctx.set_gradient_leaves(None)
                # to rounding, as test_gradient_leaf_mask_computes_only_what_is_asked_for: fewer tiles cut the K ranges differently
                assert np.allclose(masked[mask == 1], out["grad"][mask == 1], rtol=1e-11, atol=0)
                assert np.all(masked[mask == 0] == 0.0)
    sh = t.shared()
    for key, bound in (("grad", 1e-11), ("tgrad", 1e-12)):
        a, b = runs[0][key][sh], runs[1][key][sh]
        rel = np.max(np.abs(a - b), axis=1) / np.max(np.abs(b), axis=1)
        print(f"{name} {tag} {key}: shared against unshared, worst relative difference {np.max(rel):.3g} (bound {bound:g})")
        assert np.all(rel <= bound), (key, int(np.argmax(rel)), float(np.max(rel)))
    lc, lo = (t.keys.index("g300_385/" + k) for k in ("copy", "copyown")) if name == "T1" else (None, None)
    if lc is not None:          # the COPY leaf with its source's mean is its source; with a mean of its own it is not
        s = int(t.src[lc])
        assert np.allclose(runs[0]["grad"][lc], runs[0]["grad"][s], rtol=1e-12, atol=0)
        assert np.max(np.abs(runs[0]["grad"][lo] - runs[0]["grad"][s])) > 1e-6


# ------------------------------------------------------------------------------------- (d) the demoted claim

def test_prefix_claim_below_one_block_is_the_full_leaf(ctx, golden):
    """127 -> 300 copies no whole block: build_plan drops the claim.  With and without it the same results (cross-run bounds), in
    a one-lane context the same lanes and, for every other leaf, the same bits; the caller's schedule stays valid: handed in
    again after the fit it is accepted and refits to the same bits."""
    t = _table("TD")
    l0 = t.keys.index("g127_300/leaf")
    assert t.op[l0] == st.PREFIX and t.kb(l0) == 0
    op2, src2, plen2 = t.op.copy(), t.src.copy(), t.plen.copy()
    op2[l0], src2[l0], plen2[l0] = st.FULL, -1, 0
    every = list(range(t.L))
    with _Options(ctx, DEFAULTS):
        claimed = _run(ctx, t, DEFAULTS, leaves=every)
        _check_references(t, claimed, golden)
        ctx.set_sharing(t.op, t.src, t.plen)                 # the same arrays again: still a valid schedule
        ctx.set_test(t.Xt, t.route_ptr, t.route_idx)
        mll2, info2, _ = ctx.fit()
        ctx.predict_run()
        mu2, var2 = ctx.predict_fetch()
        assert _same_bits(mll2, claimed["mll"]) and np.all(info2 == 0)
        assert _same_bits(mu2, claimed["mu"]) and _same_bits(var2, claimed["var"])
        for l in every:
            F, a = ctx.download_factor(l, int(t.n[l]))
            assert _same_bits(F, claimed["fa"][l][0]) and _same_bits(a, claimed["fa"][l][1]), l
        without = _run(ctx, t, DEFAULTS, leaves=every, schedule=(op2, src2, plen2))
    assert claimed["lanes"] == without["lanes"] == 1
    worst = _check_cross(t, claimed, without, leaves=[l0])
    a, b = int(t.route_ptr[l0]), int(t.route_ptr[l0 + 1])
    assert np.allclose(claimed["mu"][a:b], without["mu"][a:b], rtol=1e-11, atol=1e-12)      # as the joint / standalone comparison
    assert np.allclose(claimed["var"][a:b], without["var"][a:b], rtol=1e-10, atol=1e-13)
    for l in every:
        if l != l0:
            assert _same_bits(claimed["fa"][l][0], without["fa"][l][0]) and _same_bits(claimed["fa"][l][1], without["fa"][l][1]), l
            assert claimed["mll"][l] == without["mll"][l]
    keep = np.ones(t.route_idx.size, dtype=bool)
    keep[a:b] = False
    assert _same_bits(claimed["mu"][keep], without["mu"][keep]) and _same_bits(claimed["var"][keep], without["var"][keep])
    print(f"\ndemoted claim against the plain leaf: worst error / bound {worst:.3g}")


# ------------------------------------------------------------------------------------- (e) refusals

def test_refused_schedules_leave_the_context_as_it_was(ctx):
    """include/dsmgp_hip.h: a rejected schedule leaves the context exactly as it was.  After a fit, predict_run and a fetch on T3
    every lie returns DSMGP_E_ARG, and predict_fetch, download_factor and a second fit return the bits from before."""
    t = _table("T3")
    L = t.L
    src_a, rep_a = [l for l, k in enumerate(t.keys) if k == "g129_130/src"]       # a source and its replica: equal lists
    pre_a = t.keys.index("g129_130/leaf")
    pre_b = t.keys.index("g300_385/leaf")
    other = t.keys.index("g300_385/src")
    assert t.kid[other] != t.kid[pre_a] and np.array_equal(t.obs[src_a], t.obs[rep_a])

    def schedule(changes):
        op, src, plen = t.op.copy(), t.src.copy(), t.plen.copy()
        for l, (o, s, p) in changes.items():
            op[l], src[l], plen[l] = o, s, p
        return op, src, plen

    n_src = int(t.n[src_a])
    lies = {
        "source is a COPY leaf": schedule({rep_a: (st.COPY, src_a, 0), pre_a: (st.PREFIX, rep_a, n_src)}),
        "source is a PREFIX leaf": schedule({pre_b: (st.PREFIX, pre_a, int(t.n[pre_a]))}),
        "prefix_len is not the source's n": schedule({pre_a: (st.PREFIX, src_a, n_src - 1)}),
        "equal lists claimed as PREFIX": schedule({rep_a: (st.PREFIX, src_a, n_src)}),
        "kernel ids differ": schedule({pre_a: (st.PREFIX, other, int(t.n[other]))}),
        "src == l": schedule({pre_a: (st.PREFIX, pre_a, n_src)}),
        "src out of range (L)": schedule({pre_a: (st.PREFIX, L, n_src)}),
        "src out of range (-1)": schedule({pre_a: (st.PREFIX, -1, n_src)}),
        "unknown op": schedule({pre_a: (3, src_a, n_src)}),
    }
    watched = t.shared() + [src_a, other]
    with _Options(ctx, DEFAULTS):
        before = _run(ctx, t, DEFAULTS, leaves=watched)
        assert np.all(before["info"] == 0)
        for what, (op, src, plen) in lies.items():
            with pytest.raises(hipabi.DsmgpError) as e:
                ctx.set_sharing(op, src, plen)
            assert e.value.code == hipabi.E_ARG, what
            mu, var = ctx.predict_fetch()
            assert _same_bits(mu, before["mu"]) and _same_bits(var, before["var"]), what
            for l in watched:
                F, a = ctx.download_factor(l, int(t.n[l]))
                assert _same_bits(F, before["fa"][l][0]) and _same_bits(a, before["fa"][l][1]), (what, l)
        mll, info, _ = ctx.fit()
        ctx.predict_run()
        mu, var = ctx.predict_fetch()
        assert _same_bits(mll, before["mll"]) and np.all(info == 0)
        assert _same_bits(mu, before["mu"]) and _same_bits(var, before["var"])
        assert ctx.work_fused()[1] == before["fused"]


# ------------------------------------------------------------------------------------- (f) a failed source

def _with_a_fifth_family(t):
    """T2 plus a family on rows of its own behind all others: a 128-row source on the rows 2^27 e_(i mod 3) and nine PREFIX leaves
    of 129 and 513..640 rows whose tails are ordinary rows, kernel id 4.  Under IsoLinear with l = 1 and a noise that 2^54
    absorbs (test_first_bad_minor_is_reported_exactly) row 3 repeats row 0 and the source's fourth pivot is exactly zero; under
    IsoSE the same rows give a well-conditioned leaf.  Phase 1 still runs steps 2-4 fused."""
    import copy
    f = copy.copy(t)
    n0 = t.X.shape[0]
    special = np.zeros((st.TB, 3))
    special[np.arange(st.TB), np.arange(st.TB) % 3] = 2.0 ** 27
    tails = st.uniform(7900, 0, 512 * 3).reshape((512, 3), order="F")
    f.X = np.asfortranarray(np.concatenate([t.X, special, tails]))
    f.y = np.concatenate([t.y, np.zeros(st.TB), np.sin(3.0 * tails[:, 0]) + tails[:, 2]])
    src = np.arange(n0, n0 + st.TB)
    sizes = [129] + st.BIG
    f.obs = t.obs + [src] + [np.arange(n0, n0 + n) for n in sizes]
    f.keys = t.keys + ["bad/src"] + [f"bad/{n}" for n in sizes]
    f.L = len(f.obs)
    f.n = np.array([o.size for o in f.obs])
    f.obs_ptr = np.concatenate([[0], np.cumsum(f.n)]).astype(np.int64)
    f.obs_idx = np.concatenate(f.obs)
    f.kid = np.concatenate([t.kid, np.full(1 + len(sizes), 4)]).astype(np.int32)
    f.mean = np.concatenate([t.mean, np.zeros(1 + len(sizes))])
    f.op = np.concatenate([t.op, [st.FULL], np.full(len(sizes), st.PREFIX)]).astype(np.int32)
    f.src = np.concatenate([t.src, [-1], np.full(len(sizes), t.L)]).astype(np.int32)
    f.plen = np.concatenate([t.plen, [0], np.full(len(sizes), st.TB)]).astype(np.int64)
    f.routes = t.routes + [t.routes[0][:0]] + [np.arange(16, dtype=np.int64)] * len(sizes)
    f.route_ptr = np.concatenate([[0], np.cumsum([r.size for r in f.routes])]).astype(np.int64)
    f.route_idx = np.concatenate(f.routes)
    f.hyper = dict(t.hyper)
    assert st.fused_steps(f.n, f.op, f.plen) == t.fused and t.fused[1]
    return f


def test_prefix_leaves_of_a_failed_source(ctx):
    """include/dsmgp_hip.h (dsmgp_fit): the PREFIX leaves of a source whose factorisation failed inside the rows they copy
    report the source's info -- the same leading minor is their own first bad one, LAPACK's value -- and get NaN wherever a
    failed leaf does (dsmgp_solve_targets, dsmgp_predict_targets, dsmgp_loo, dsmgp_predict_gradients); every other leaf keeps
    the bits it has when that source does not fail."""
    t = _with_a_fifth_family(st.table("T2"))
    fam = [l for l in range(t.L) if t.kid[l] == 4]
    s0, pre = fam[0], fam[1:]
    rest = [l for l in range(t.L) if t.kid[l] != 4]
    Xs = t.X[t.obs[s0]]
    _, linfo = sla.lapack.dpotrf(Xs @ Xs.T + (np.exp(-60.0) + 1e-8) * np.eye(st.TB), lower=1)
    assert linfo == 4
    Y = np.stack([t.y, np.cos(t.X[:, 0]), t.y + 1.0], axis=1)
    watch = rest[:6] + t.leaves(st.PREFIX)[:6]

    def run(kind, hyp):
        t.hyper[4] = (kind, np.asarray(hyp))
        r = _run(ctx, t, DEFAULTS, leaves=watch, references=False)
        r["tmll"], _ = ctx.solve_targets(Y)
        r["tmu"] = ctx.predict_targets()
        r["loo"] = ctx.loo()
        r["dmu"], r["dvar"] = ctx.predict_gradients()
        return r

    with _Options(ctx, DEFAULTS):
        good = run(0, [np.log(0.3), 0.0, np.log(0.1)])
        bad = run(2, [0.0, 0.0, -30.0])
    assert np.all(good["info"] == 0) and good["fused"] > 0 and bad["fused"] == good["fused"]
    print(f"\ninfo of the failed source and its PREFIX leaves: {bad['info'][fam].tolist()}")
    assert bad["info"][s0] == linfo and np.all(bad["info"][pre] == linfo) and np.all(bad["info"][rest] == 0)
    ent = np.zeros(t.route_idx.size, dtype=bool)
    row = np.zeros(t.obs_idx.size, dtype=bool)
    for l in fam:
        ent[t.route_ptr[l]:t.route_ptr[l + 1]] = True
        row[t.obs_ptr[l]:t.obs_ptr[l + 1]] = True
    assert np.all(np.isnan(bad["tmll"][fam])) and np.all(np.isnan(bad["tmu"][ent]))
    assert np.all(np.isnan(bad["loo"][0][row])) and np.all(np.isnan(bad["loo"][1][row])) and np.all(np.isnan(bad["loo"][2][fam]))
    assert np.all(np.isnan(bad["dmu"][ent])) and np.all(np.isnan(bad["dvar"][ent]))
    assert _same_bits(bad["mll"][rest], good["mll"][rest])
    for k in ("mu", "var", "tmu", "dmu", "dvar"):
        assert _same_bits(bad[k][~ent], good[k][~ent]), k
    assert _same_bits(bad["tmll"][rest], good["tmll"][rest]) and _same_bits(bad["loo"][2][rest], good["loo"][2][rest])
    assert _same_bits(bad["loo"][0][~row], good["loo"][0][~row]) and _same_bits(bad["loo"][1][~row], good["loo"][1][~row])
    for l in watch:
        assert _same_bits(bad["fa"][l][0], good["fa"][l][0]) and _same_bits(bad["fa"][l][1], good["fa"][l][1]), l
