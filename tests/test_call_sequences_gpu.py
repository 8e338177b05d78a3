"""GPU suite: every entry point's result is pinned to its inputs, whatever ran before it.

The committed sequences of tests/call_sequences.py (tests/golden/call_sequences.json) run one after the other on ONE long-lived
hipabi.Context -- through the wrapper, so its cached L, D, n_obs, leaf_n, route_total, n_t and targets_Q are under test too --
with the state model and the dense float64 oracle chain (tests/call_sequences_oracle.py) kept in step.  At every reader:

1. bits     the result has the uint64 view of the same reader on a fresh hipabi.Context(0) brought to the same inputs and the
            same path-defining state by the shortest route (call_sequences.route) and closed afterwards.  Fresh results are kept
            by call_sequences.Model.path_key: a fresh context's answer does not depend on the history it is compared with.
2. dense    the fresh context's result agrees with the dense reference at the tolerance the named helper derives, doubled
            (both sides float64): no new constant.  This excludes both contexts being wrong in the same way.
3. refusal  where the model says the reader's chain is broken the call returns DSMGP_E_STATE, a deliberately bad argument
            DSMGP_E_ARG, and the readers that follow still get their bits.
4. poison   under the hyper-vector that fails one leaf, the calls the header promises NaN rows for give NaN exactly there and
            the other leaves keep their bits; after the healthy vector and a refit everything is clean again.

Documented path differences, reproduced by the route (so bits still apply): a fit that carries a resident test set runs other
task lists than a fit alone (include/dsmgp_hip.h: "While a test set is resident (dsmgp_set_test), dsmgp_fit also advances its
rows through the factorisation launches"; the order of split-K pieces differs), so the route registers the set the last fit
carried before its fit; and K_tn L^-T of rows registered later comes from the standalone sweep.  No other difference is listed:
an unlisted one is a failure.

Nothing is retried.  Before each op the test overwrites `last_op.txt` under tmp_path with the sequence id, the op index and the
op: after a fault, abort or hang the culprit is read from that file and from `python -m tests.call_sequences --print ID`.

Cost on an MI355X (measured, one run of the file): about 700 fresh-context replays (create, route, reader, close) of 0.03 s
each on average -- the others are answered from the results kept by path -- 31 s for the 97 tests of the file, the longest of
them (table W, 40 leaves) 3.3 s.
"""
import copy
import time

import numpy as np
import pytest

import call_sequences as cs
from call_sequences_oracle import Harness
from deepstructuredmixtures_amd import hipabi

pytestmark = pytest.mark.gpu

SEQS = cs.committed()
# what include/dsmgp_hip.h promises NaN for on a leaf whose fit reported info != 0
NAN_PROMISED = ("predict_gradients", "loo", "loo_gradients", "solve_targets", "predict_targets", "targets_gradients", "loo_targets",
                "loo_targets_gradients")


class Run:
    """The long-lived context with the model and the oracle in step; replaced as a whole after a test failed half way."""

    def __init__(self):
        self.ctx = hipabi.Context(0)
        self.h = Harness()
        self.h.start()
        self.dirty = False

    def close(self):
        self.ctx.close()


@pytest.fixture(scope="module")
def shared():
    s = dict(run=None, fresh={}, replay_seconds=0.0, replays=0, t0=time.time())
    yield s
    if s["run"] is not None:
        s["run"].close()
    n = max(1, s["replays"])
    print(f"\ncall sequences: {s['replays']} fresh-context replays, {s['replay_seconds'] / n:.3f} s each on average, "
          f"{time.time() - s['t0']:.1f} s for the file")


def _same_bits(a, b, healthy=None, info=False):
    """The same uint64 view (NaN in the same places).  `healthy`: under the poison vector, the entries of the leaves whose fit
    succeeded -- what the failed leaf's entries hold beside the promised NaN is not defined, so only those are compared;
    `info`: the fit's info array, whose value on the failed leaf is compared as zero / nonzero then.  Every other integer result
    (the routes) is compared exactly."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return bool(np.array_equal(a != 0, b != 0) if (info and healthy is not None) else np.array_equal(a, b))
    if healthy is not None:
        a, b = a[healthy], b[healthy]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a[~na]).view(np.uint64),
                                                           np.ascontiguousarray(b[~nb]).view(np.uint64)))


def _replay(shared, before, call):
    """`call` on a fresh context brought to the state of `before` by the shortest route."""
    t = time.perf_counter()
    c = hipabi.Context(0)
    try:
        m = cs.Model()
        for op, arg in cs.route(before, call):
            cs.run_op(c, m, op, arg)
            assert m.apply(op, arg) is None, (op, arg)
        out = cs.read(c, m, call)
    finally:
        c.close()
    shared["replay_seconds"] += time.perf_counter() - t
    shared["replays"] += 1
    return tuple(np.array(a, copy=True) for a in out)


def _check_nan_rows(tag, name, k, g, fin):
    """4. poison: where the reference marks the failed leaf (`fin` false), a reader the header promises NaN for gives NaN."""
    if name not in NAN_PROMISED:
        return
    if name.endswith("gradients") and k == 0:
        # a NaN row over the failed leaf's hyper-vector; past it the header allows the zeros every row has there
        nh = len(cs.POISON[1])
        bad = ~fin.all(axis=1)
        assert np.all(np.isnan(g[bad, :nh])) and np.all(np.isnan(g[bad, nh:]) | (g[bad, nh:] == 0)), (tag, k, g[bad])
    else:
        assert np.all(np.isnan(g[~fin])), (tag, k, "rows of the failed leaf must be NaN")


def _check_dense(tag, call, got, pairs, poisoned):
    assert len(got) == len(pairs), (tag, len(got), len(pairs))
    name = cs.split(call)[0]
    worst = 0.0
    for k, (g, (ref, tol)) in enumerate(zip(got, pairs)):
        g, ref = np.asarray(g), np.asarray(ref)
        assert g.shape == ref.shape, (tag, k, g.shape, ref.shape)
        if tol is None:
            assert np.array_equal(g != 0, ref != 0) if name == "fit" else np.array_equal(g, ref), (tag, k)
            continue
        tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
        fin = np.isfinite(ref)
        if not poisoned:
            assert np.all(fin), (tag, k)
        else:
            _check_nan_rows(tag, name, k, g, fin)
        assert np.all(np.isfinite(g[fin])), (tag, k)
        err = np.abs(g[fin] - ref[fin])
        if err.size:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(tol[fin] > 0, err / tol[fin], np.where(err > 0, np.inf, 0.0))      # tolerance 0: an exact zero
            worst = max(worst, float(np.max(ratio)))
            w = int(np.argmax(ratio))
            assert np.all(err <= tol[fin]), (tag, k, float(g[fin][w]), float(ref[fin][w]), float(tol[fin][w]), float(ratio[w]))
    return worst


def _defaults(run, crumb):
    """Bring options, the joint switch and the pool back to their defaults: each sequence was generated from them."""
    m = run.h.m
    ops = [["set_option", [k, v]] for k, v in sorted(cs.OPT_DEFAULT.items()) if m.opts[k] != v]
    ops += ([["set_joint", 1]] if not m.joint else []) + ([["reserve", 0]] if m.reserved else [])
    for op, arg in ops:
        crumb(-1, op, arg)
        cs.run_op(run.ctx, copy.deepcopy(m), op, arg)
        run.h.step(op, arg)


@pytest.mark.parametrize("seq", SEQS, ids=[s["id"] for s in SEQS])
def test_sequence(shared, tmp_path, seq):
    if shared["run"] is None or shared["run"].dirty:
        if shared["run"] is not None:
            shared["run"].close()
        shared["run"] = Run()
    run = shared["run"]
    run.dirty = True            # until the sequence has run to its end
    path = tmp_path / "last_op.txt"

    def crumb(i, op, arg):
        path.write_text(f"{seq['id']} {i} {op} {arg!r}\n")

    try:
        _run_sequence(shared, run, seq, crumb)
    except hipabi.DsmgpError as e:
        if e.code == hipabi.E_HIP:      # the device reported an error: nothing more is started on it from this process
            pytest.exit(f"HIP error in {path.read_text().strip()}: {e}", returncode=3)
        raise
    run.dirty = False


def _run_sequence(shared, run, seq, crumb):
    ctx, h = run.ctx, run.h
    _defaults(run, crumb)
    worst, checked, refused = 0.0, 0, 0
    for i, (op, arg) in enumerate(seq["ops"]):
        tag = f"{seq['id']}[{i}] {op} {arg!r}"
        crumb(i, op, arg)
        code, call, pairs, before = h.step(op, arg)
        if code is not None:                                    # 3. refusals
            with pytest.raises(hipabi.DsmgpError) as ei:
                cs.run_op(ctx, before, op, arg)
            assert ei.value.code == code, (tag, ei.value.code, str(ei.value))
            refused += 1
            continue
        got = cs.run_op(ctx, before, op, arg)
        if op == "fit" and before.leaves == "W" and before.opts["fused_steps"] and before.opts["fused_gram"]:
            assert ctx.work_fused()[1] > 0, tag                 # >= 32 leaves in the shallow block steps: they run fused
        if call is None:
            continue
        key = before.path_key(call)
        poisoned = before.poisoned
        if key not in shared["fresh"]:
            fresh = _replay(shared, before, call)
            worst = max(worst, _check_dense(tag + " fresh against dense", call, fresh, pairs, poisoned))       # 2. dense
            shared["fresh"][key] = fresh
        fresh = shared["fresh"][key]
        assert len(got) == len(fresh), tag
        for k, (a, b) in enumerate(zip(got, fresh)):                                                         # 1. bits
            healthy = np.isfinite(np.asarray(pairs[k][0], dtype=np.float64)) if poisoned else None
            if poisoned and pairs[k][1] is not None:           # 4. the long-lived context's own NaN rows, not only the fresh one's
                _check_nan_rows(tag + " long-lived context", cs.split(call)[0], k, np.asarray(a), healthy)
            assert _same_bits(a, b, healthy, info=op == "fit"), (tag, k, "differs from a fresh context on " + repr(cs.route(before, call)),
                                      float(np.nanmax(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))
                                      if np.asarray(a).shape == np.asarray(b).shape and np.asarray(a).size else None)
        checked += 1
    print(f"\n{seq['id']}: {checked} readers bit-equal to a fresh context, {refused} refusals, worst dense err/tol {worst:.3g}")
