"""GPU suite: the device routing chain (dsmgp_set_tree + dsmgp_set_test_routed: route_walk_kernel<false>, scan_counts_kernel
twice, route_rank_kernel, route_fill_kernel, route_walk_kernel<true>) at its scan, bitmap-word and stack edges, against the
NumPy recursion of tests/routing_cases.py -- a reference that shares nothing with csrc/route_walk.hpp.  tests/test_routing_host.py
shows on the CPU that every case crosses the edge it is named for and that the reference is right.

CSR comparisons are exact.  The per-row entry index (row_ptr / row_ent / ent_leaf) has no download of its own: it is pinned
through everything that walks it, bit for bit against the host-built index of dsmgp_set_test, and against
pred_tolerance.aggregate on the reference's own per-row entries within pred_tolerance.agg_tol."""
import numpy as np
import pytest

from deepstructuredmixtures_amd import hipabi
from pred_tolerance import agg_tol, aggregate, moment_tol
from predsample_dense import same_bits
import routing_cases as rc

pytestmark = pytest.mark.gpu

LOG_ELL = {3: np.log(30.0), 1: np.log(0.7)}       # tree A's thresholds span [-50, 50], tree B's rows [-1, 1]
LOG_SF, LOG_NOISE = 0.0, np.log(0.3)


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _leaf_table(ctx, L, D):
    """The smallest leaves the table takes -- 2 or 3 training rows each, IsoSE -- with a distinct mean per leaf, so that the
    moments of two leaves cannot be taken for one another.  Returns the per-leaf means and the targets."""
    n = 2 + np.arange(L) % 2
    ptr = np.concatenate([[0], np.cumsum(n)])
    rng = np.random.default_rng(7000 + L)
    X = rng.uniform(-50.0 if D == 3 else -1.0, 50.0 if D == 3 else 1.0, size=(int(ptr[-1]), D))
    mean = 0.5 + 0.01 * np.arange(L)
    y = np.repeat(mean, n) + 0.3 * rng.standard_normal(int(ptr[-1]))
    ctx.set_train(X, y)
    ctx.set_leaves(ptr, np.arange(int(ptr[-1])), np.zeros(L, dtype=np.int32), mean)
    ctx.set_hyper(0, 0, [LOG_ELL[D], LOG_SF, LOG_NOISE])
    return mean, y


def _set(ctx, tree):
    _leaf_table(ctx, tree.n_leaves, tree.D)
    ctx.set_tree(*tree.arrays())


def _routed_is_exact(ctx, Xt, ref):
    ptr, idx = ref[0], ref[1]
    got = ctx.set_test_routed(Xt)
    gp, gi = ctx.routes()
    assert np.array_equal(got, ptr) and np.array_equal(gp, ptr) and np.array_equal(gi, idx)


@pytest.mark.parametrize("tree_name,rows", [(t, r) for t, sets in rc.ROW_SETS_OF.items() for r in sets])
def test_device_csr_equals_the_reference_at_every_size(ctx, tree_name, rows):
    """Every n_t of routing_cases.N_T, in ascending order on one context: 1, around one word, around the scans' 1024, around the
    rank kernel's 8192 rows, a multiple of 32 past it, and two rank chunks plus one row."""
    _set(ctx, rc.case(tree_name, rows, 1).tree)
    for n_t in rc.N_T:
        c = rc.case(tree_name, rows, n_t)
        ref = rc.reference(tree_name, rows, n_t)
        rc.assert_case_reaches_its_edge(c, ref)
        _routed_is_exact(ctx, c.Xt, ref)


def test_workspace_reuse_after_a_larger_set(ctx):
    """rws_counts and rws_bits grow with slack and are kept: a smaller set after a larger one reads a workspace that still holds
    the larger one's bits and counts behind its own."""
    _set(ctx, rc.tree_a())
    for rows, n_t in (("spread", 16385), ("edges", 33), ("spread", 8193), ("one_child", 2048), ("spread", 1025)):
        _routed_is_exact(ctx, rc.case("A", rows, n_t).Xt, rc.reference("A", rows, n_t))


def test_refused_registration_leaves_nothing_behind(ctx):
    """A NaN in the first row, in a row on the scan's chunk edge and in the last row; +inf beyond a finite last threshold."""
    _set(ctx, rc.tree_a())
    good = rc.case("A", "spread", 2048)
    for row, d in ((1024, 0), (0, 1), (2047, 2)):
        _routed_is_exact(ctx, good.Xt, rc.reference("A", "spread", 2048))
        bad = good.Xt.copy()
        bad[row, d] = np.nan
        with pytest.raises(ValueError, match="outside"):
            rc.route_reference(good.tree, bad)
        with pytest.raises(hipabi.DsmgpError, match="outside"):
            ctx.set_test_routed(bad)
        with pytest.raises(hipabi.DsmgpError, match="before set_test"):
            ctx.routes()
        small = rc.case("A", "edges", 33)                                    # ... and a smaller set on the workspace it left
        _routed_is_exact(ctx, small.Xt, rc.reference("A", "edges", 33))
    finite = rc.flatten("finite", ("split", 2, [0.0, 1.0], [("leaf", 0), ("leaf", 1)]), 1200, 3)
    ctx.set_tree(*finite.arrays())
    Xt = np.zeros((1025, 3))
    Xt[:, 2] = np.where(np.arange(1025) % 2, 1.0, -np.inf)
    _routed_is_exact(ctx, Xt, rc.route_reference(finite, Xt))
    Xt[1024, 2] = np.inf
    with pytest.raises(hipabi.DsmgpError, match="outside"):
        ctx.set_test_routed(Xt)
    with pytest.raises(hipabi.DsmgpError, match="before set_test"):
        ctx.routes()
    Xt[1024, 2] = 1.0
    _routed_is_exact(ctx, Xt, rc.route_reference(finite, Xt))


def test_stack_of_96_is_filled_and_97_is_refused(ctx):
    b, bplus = rc.tree_b(), rc.tree_b(1)
    _set(ctx, b)
    ref = rc.reference("B", "all", 1025)
    assert np.all(ref[2].counts() == rc.ROUTE_STACK)
    _routed_is_exact(ctx, rc.case("B", "all", 1025).Xt, ref)
    with pytest.raises(hipabi.DsmgpError, match=r"needs 97 pending.*holds 96") as e:
        ctx.set_tree(*bplus.arrays())
    assert e.value.code == hipabi.E_ARG
    _routed_is_exact(ctx, rc.case("B", "all", 33).Xt, rc.reference("B", "all", 33))     # tree B is still the context's tree


@pytest.mark.parametrize("which", ["order", "twice"])
def test_trees_the_device_cannot_represent_are_refused(ctx, which):
    """The device path keeps one bit per (leaf, row) and writes a row's entries in visit order: a leaf named twice, or leaves not
    numbered depth-first, cannot give the index dsmgp_set_test builds from the host routine's lists
    (test_what_the_host_routine_does_with_the_trees_the_device_cannot_represent), so dsmgp_set_tree refuses them."""
    _set(ctx, rc.tree_a())
    small = rc.case("A", "edges", 33)
    _routed_is_exact(ctx, small.Xt, rc.reference("A", "edges", 33))
    with pytest.raises(hipabi.DsmgpError, match={"order": "depth-first", "twice": "twice"}[which]) as e:
        ctx.set_tree(*rc.tree_c(which).arrays())
    assert e.value.code == hipabi.E_ARG
    _routed_is_exact(ctx, small.Xt, rc.reference("A", "edges", 33))                      # the previous tree still routes


def _consumers(ctx, L, y_test, D):
    """Everything that walks the per-row entry index, after predict_run: (name -> arrays)."""
    ctx.predict_run()
    out = {"moments": ctx.predict_fetch()}
    coef = 0.2 + 0.1 * (np.arange(L) % 7)
    group = (np.arange(L) % 4).astype(np.int32)
    for name, fam, kw in (("mixture", hipabi.AGG_MIXTURE, dict(leaf_coef=coef)), ("poe", hipabi.AGG_POE, dict(leaf_coef=np.ones(L))),
                          ("gpoe", hipabi.AGG_GPOE, dict(leaf_coef=coef)), ("rbcm", hipabi.AGG_RBCM, dict(leaf_group=group, n_groups=4))):
        out[name] = ctx.aggregate(fam, **kw)
        out[name + " gradients"] = ctx.aggregate_gradients()
        out[name + " scores"] = (np.array(list(ctx.scores(y_test).values())),)
    return out, coef, group


CONSUMER_CASES = [("A", "spread", 1025), ("A", "spread", 8193), ("A-shard", "spread", 1025), ("B", "all", 1025)]
FAMILIES = {"mixture": hipabi.AGG_MIXTURE, "poe": hipabi.AGG_POE, "gpoe": hipabi.AGG_GPOE, "rbcm": hipabi.AGG_RBCM}
_RUNS = {}


def _both_registrations(ctx, tree_name, rows, n_t):
    """One fit, two registrations of the same rows -- routed on the device, and dsmgp_set_test with the reference's CSR (its
    per-row index is built on the host, by ascending leaf) -- and what every consumer gives on each.  Once per case."""
    key = (tree_name, rows, n_t)
    if key not in _RUNS:
        tree = rc.case(*key).tree
        Xt = rc.rows_spread(n_t, finite=True) if rows == "spread" else rc.case(*key).Xt
        ptr, idx, ent = rc.route_reference(tree, Xt)
        _, y = _leaf_table(ctx, tree.n_leaves, tree.D)
        ctx.set_tree(*tree.arrays())
        _, info, _ = ctx.fit()
        assert np.all(info == 0)
        y_test = 0.5 + np.sin(np.arange(n_t))
        _routed_is_exact(ctx, Xt, (ptr, idx))
        routed, coef, group = _consumers(ctx, tree.n_leaves, y_test, tree.D)
        ctx.set_test(Xt, ptr, idx)
        hosted, _, _ = _consumers(ctx, tree.n_leaves, y_test, tree.D)
        _RUNS[key] = dict(ent=ent, routed=routed, hosted=hosted, coef=coef, group=group, yscale=max(1.0, float(np.max(np.abs(y)))))
    return _RUNS[key]


@pytest.mark.parametrize("tree_name,rows,n_t", CONSUMER_CASES)
def test_entry_index_gives_the_bits_of_the_host_built_index(ctx, tree_name, rows, n_t):
    """Moments, the four aggregates, their input gradients and the scores: the same bits from both registrations (same entry
    index, same summation order), rows that reach no held leaf (the shard) included."""
    run = _both_registrations(ctx, tree_name, rows, n_t)
    assert set(run["routed"]) == {"moments"} | {f + s for f in FAMILIES for s in ("", " gradients", " scores")}
    for name in run["routed"]:
        for a, b in zip(run["routed"][name], run["hosted"][name]):
            assert same_bits(a, b), (name, int(np.sum(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))))


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("tree_name,rows,n_t", CONSUMER_CASES)
def test_entry_index_against_the_reference_entries(ctx, tree_name, rows, n_t, family):
    """The routed registration's aggregate must be pred_tolerance.aggregate of the fetched per-entry moments over the REFERENCE's
    per-row entries, within pred_tolerance.agg_tol (the project's bound, the fetched moments taken at moment_tol) -- which a
    wrong entry index fails even if it reached both registrations.  Rows without entries are left to the bit comparison."""
    run = _both_registrations(ctx, tree_name, rows, n_t)
    ent, coef, group = run["ent"], run["coef"], run["group"]
    mu, var = run["routed"]["moments"]
    assert np.all(np.isfinite(mu)) and np.all(var > 0)
    has = np.flatnonzero(ent.counts() > 0)
    assert has.size == n_t or (tree_name == "A-shard" and 0 < has.size < n_t)
    ent_has = [ent[r] for r in has]
    kss, noise = np.exp(2 * LOG_SF), np.exp(2 * LOG_NOISE)
    tmu, tvar = moment_tol(mu, var, np.full(mu.size, kss), noise, run["yscale"])
    fam = FAMILIES[family]
    kw = {"mixture": dict(coef=coef), "poe": dict(coef=np.ones(coef.size)), "gpoe": dict(coef=coef),
          "rbcm": dict(group=group, G=4, kss_prior=np.full(has.size, kss), noise_prior=noise)}[family]
    rm, rv = aggregate(fam, mu, var, ent_has, log=np.log, **kw)
    S1 = [sum(coef[l] * mu[e] ** 2 for l, e in er) for er in ent_has] if family == "mixture" else None
    tm, tv = agg_tol(fam, mu, var, tmu, tvar, ent_has, S1=S1, **kw)
    gm, gv = run["routed"][family]
    em, ev = np.abs(gm[has] - np.array(rm, dtype=np.float64)), np.abs(gv[has] - np.array(rv, dtype=np.float64))
    print(f"\n{tree_name} {n_t} {family}: worst err/tol mu {np.max(em / tm):.3g} var {np.max(ev / tv):.3g}")
    assert np.all(em <= tm) and np.all(ev <= tv)
