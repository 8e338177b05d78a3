"""CPU suite of the call sequences (tests/call_sequences.py): the committed list is what the generator yields and satisfies the
coverage conditions; the state model refuses exactly what include/dsmgp_hip.h says needs an earlier call; and the whole list
runs on the dense float64 oracle chain (tests/call_sequences_oracle.py) with every reference finite for every healthy leaf and
cond_2(K_y) of every pool configuration where the tolerance helpers hold."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import call_sequences as cs
from pred_tolerance import EPS, RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _coverage():
    return cs.coverage(cs.committed())


def test_the_module_is_pure_host():
    """Importing it brings in neither the ctypes binding nor torch (a fresh interpreter: this process has both already)."""
    code = "import sys; sys.path.insert(0, 'tests'); import call_sequences; " \
           "bad = [m for m in sys.modules if m == 'torch' or m.endswith('hipabi')]; assert not bad, bad"
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


def test_constants_are_the_binding_s():
    from deepstructuredmixtures_amd import hipabi
    assert (cs.E_ARG, cs.E_STATE) == (hipabi.E_ARG, hipabi.E_STATE)
    assert cs.OPT == dict(ard=hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, fused_gram=hipabi.OPT_FUSED_GRAM, fused_steps=hipabi.OPT_FUSED_STEPS,
                          diag_in_update=hipabi.OPT_DIAG_IN_UPDATE, fit_graph=hipabi.OPT_FIT_GRAPH, lanes=hipabi.OPT_LANES)
    assert cs.FAMILY == dict(mixture=hipabi.AGG_MIXTURE, poe=hipabi.AGG_POE, gpoe=hipabi.AGG_GPOE, rbcm=hipabi.AGG_RBCM)


def test_the_committed_list_is_what_the_generator_yields():
    """Seeded, no clock, no hash(): two runs agree with each other and with tests/golden/call_sequences.json."""
    a, b = cs.generate(), cs.generate()
    assert a == b
    assert a == cs.committed(), "run `python -m tests.call_sequences --write` and review the difference"
    ids = [s["id"] for s in a]
    assert len(set(ids)) == len(ids) and all(re.fullmatch(r"[A-Za-z0-9_.-]+", i) for i in ids)


def test_the_pools_have_a_value_on_each_side_of_every_granule():
    n = {k: np.diff(cs.leaves(k)["obs_ptr"]) for k in "SWT"}
    assert sorted(n["S"][:6]) == [1, 100, 128, 129, 257, 300] and n["S"][6] == 129 and n["S"][7] == 300
    S = cs.leaves("S")
    assert np.array_equal(S["obs"][6], S["obs"][3]) and np.array_equal(S["obs"][7][:129], S["obs"][3]) and len(set(S["kid"])) == 2
    assert list(S["kid"]).count(cs.POISON_KID) == 1
    assert n["W"].size == 40 and n["W"].min() >= 130 and n["W"].max() <= 260 and n["T"].tolist() == [300]
    for k in "SWT":
        assert all(np.all(np.diff(o) > 0) and o[-1] < 1200 for o in cs.leaves(k)["obs"])
    pads = {k: sorted({-(-int(v) // cs.TB) for v in n[k]}) for k in n}
    assert pads["S"] == [1, 2, 3] and pads["T"] == [3]
    assert [-(-q // cs.TQ) for q in sorted(cs.TARGET_Q.values())] == [1, 1, 1, 2]
    counts = {k: cs.test_counts(k, 8) for k in cs.TEST_KEYS[:-1]}
    assert max(counts["t0"]) == 0 and set(counts["t1"]) == {1} and max(counts["t15"]) == 15 and max(counts["t40"]) == 40
    assert any(129 <= c <= 200 for c in counts["t200"]) and max(counts["t200"]) > cs.TB >= max(counts["t40"])
    assert [cs.TRAIN[k][:2] for k in "AB"] == [(1500, 2), (1200, 5)]
    for key in cs.TEST_KEYS[1:-1]:                      # no test row is left without a leaf
        Xt, ptr, idx = cs.testset(key, "S", 2)
        assert set(idx.tolist()) == set(range(Xt.shape[0])) and all(np.all(np.diff(idx[a:b]) > 0) for a, b in zip(ptr, ptr[1:]))
    Xt, ptr, idx = cs.routed_testset(2)
    assert ptr[-1] == 2 * Xt.shape[0] and np.diff(ptr)[[0, 4, 6]].tolist() == [0, 0, 0]


def test_every_writer_comes_right_before_every_reader():
    """For every writer w and reader r some sequence holds w, then nothing but r's minimal prerequisites, then r."""
    want = {(w, r) for w in cs.WRITERS for r in cs.READERS}
    assert not want - _coverage()["writer_reader"], sorted(want - _coverage()["writer_reader"])


def test_every_ordered_pair_of_readers_that_share_an_arena_or_a_flag_runs_back_to_back():
    want = {(a, b) for rs in cs.SHARING.values() for a in rs for b in rs if a != b}
    assert all(r in cs.READERS for rs in cs.SHARING.values() for r in rs)
    assert not want - _coverage()["pairs"], sorted(want - _coverage()["pairs"])


def test_every_sized_quantity_grows_and_shrinks_before_the_readers_that_depend_on_it():
    want = {(q, o, r) for q in cs.SIZED for o in ("grow-shrink", "shrink-grow") for r in cs.SIZED_FAMILIES[q]}
    assert set(cs.SIZED) == {"npad", "L", "D", "Qpad", "test_rows", "route_total"}
    assert not want - _coverage()["sized"], sorted(want - _coverage()["sized"])


def test_every_broken_chain_appears_with_the_refusal_expected():
    want = cs.expected_broken()
    assert ("fit", "scores") in want and ("set_hyper_values", "aggregate_finish") in want      # the staleness this suite started from
    assert ("set_joint", "loo") not in want
    assert not want - _coverage()["broken"], sorted(want - _coverage()["broken"])


def test_the_model_refuses_exactly_what_the_header_says_needs_an_earlier_call():
    """Stage by stage from an empty context: after each call, the readers that answer are those whose NEEDS are met, and NEEDS
    is the header's wording (the table in tests/call_sequences.py quotes it)."""
    stages = [("set_train", "A", set()), ("set_leaves", "S", set()), ("set_hyper", [0, "isose", "a"], set()),
              ("set_hyper", [1, "ardse", "a"], {"kernel_matrix", "fit"}),
              ("fit", None, {"kernel_matrix", "fit", "download_factor", "gradients", "loo", "loo_gradients", "solve_targets"}),
              ("set_test", "t15", {"routes"}), ("predict_run", None, {"predict_fetch", "predict_cov", "predict_gradients", "aggregate",
                                                                       "aggregate_partial"}),
              ("solve_targets", "q3", {"targets_fetch", "predict_targets", "targets_gradients", "loo_targets", "loo_targets_gradients"}),
              ("aggregate_partial", "poe", {"aggregate_finish"}), ("aggregate_finish", None, {"scores"})]
    m, answered = cs.Model(), set()
    assert not any(m.has(w) for w in ("leaves", "fit", "test", "pred", "targets", "partial", "done"))
    for op, arg, more in stages:
        assert m.apply(op, arg) is None, (op, arg)
        answered |= more
        assert {r for r in cs.NEEDS if m.ready(r)} == answered, (op, sorted(answered))
    assert set(cs.NEEDS) == {cs.split(r)[0] for r in cs.READERS} and cs.EXCEPTIONS == {}
    # a fit or new hyper-parameters break prediction, targets and aggregation together; the test set and the routes stay
    for op, arg, kept in (("fit", None, {"routes", "kernel_matrix", "fit", "download_factor", "gradients", "loo", "loo_gradients",
                                         "solve_targets"}), ("set_hyper", [0, "isose", "b"], {"routes", "kernel_matrix", "fit"})):
        assert m.apply(op, arg) is None
        assert {r for r in cs.NEEDS if m.ready(r)} == kept, (op, sorted(r for r in cs.NEEDS if m.ready(r)))
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    for words in ("Needs dsmgp_predict_run on the current fit (DSMGP_E_STATE otherwise)", "Needs a fit (DSMGP_E_STATE otherwise)",
                  "Needs a fit and a dsmgp_solve_targets on the CURRENT fit (DSMGP_E_STATE otherwise)",
                  "Needs BOTH dsmgp_solve_targets and dsmgp_predict_run on the CURRENT fit",
                  "A later dsmgp_fit or dsmgp_set_hyper makes them stale"):
        assert words in header, words


def test_the_route_is_the_shortest_and_reproduces_the_path():
    """After a long history the route holds each setter once, the test set before the fit only when the last fit carried one,
    and brings a fresh model to the same inputs and path."""
    for seq in cs.committed():
        m = cs.Model()
        for op, arg in seq["ops"]:
            call = cs.call_id(op, arg)
            if call is not None and m.ready(call) and not (op == "aggregate_finish" and m.agg is None):
                ops = cs.route(m, call)
                names = [o for o, _ in ops]
                assert names.count("set_train") == 1 and names.count("fit") <= 1 and names.count("set_leaves") <= 1
                f = cs.Model()
                for o, a in ops:
                    assert f.apply(o, a) is None, (seq["id"], call, o, a)
                assert f.ready(call) and f.path_key(call) == m.path_key(call), (seq["id"], call, ops)
                if "fit" in names and op != "fit":
                    assert ("set_test" in names[:names.index("fit")]) == (m.fit_test is not None), (seq["id"], call, ops)
            m.apply(op, arg)


# What each writer class does to the products of csrc/ctx_state.hpp: (invalidated, marked), read off the entry point in
# csrc/dsmgp_hip.cpp and the free_* functions it calls.  No row: refused (argument checks only) and the poison pair (a set_hyper).
_FREE_GRAD = ("grad_lists", "xinv", "loo_lists", "lg_lists")
_NEW_PLAN = (("plan",), ())                                     # free_plan_and_test
CTX_WRITES = {"set_train": (("plan", "routing_tree"), ()), "set_leaves": (("plan", "routing_tree"), ()), "set_sharing": _NEW_PLAN,
              "set_hyper_values": (("fit",), ()), "set_hyper_kind": (_FREE_GRAD + ("fit",), ()),
              "set_test": (("test",), ("test",)), "set_test_routed": (("test",), ("routing_tree", "test")),
              "set_joint": ((), ()), "opt_ard": (_FREE_GRAD, ()), "opt_fused_gram": _NEW_PLAN, "opt_fused_steps": _NEW_PLAN,
              "opt_lanes": _NEW_PLAN, "opt_diag_in_update": _NEW_PLAN, "opt_fit_graph": ((), ()),
              "set_gradient_leaves": (("grad_lists",), ()), "reserve": _NEW_PLAN, "release": _NEW_PLAN,
              "fit": (("fit",), ("fit",)), "predict_run": (("prediction",), ("vt", "prediction")),
              "solve_targets": (("targets",), ("targets",))}
CTX_WORD = {"fit": "fit", "test": "test", "pred": "prediction", "targets": "targets", "partial": "partial", "done": "done"}
CTX_POOL_STACK = _FREE_GRAD + ("target_lists",)     # free_test under a reserved pool: what is carved above the test arenas goes too


def test_the_context_s_dependency_table_is_the_model_s(tmp_path):
    """csrc/ctx_state.hpp, printed by tests/ctx_state_dump.cpp, against Model.apply: from a context where everything is current,
    with and without a reserved pool, one instance of every writer class fells a has() word of the model if and only if the
    word's product falls with what the writer invalidates (and is not marked again by it); a product is only marked while its
    parents are current; and every product is a root or falls with another."""
    exe = str(tmp_path / "ctx_state_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ctx_state_dump.cpp"), "-o", exe], check=True)
    import json
    table = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert set(CTX_WORD.values()) | set(CTX_POOL_STACK) <= set(table)
    assert all(set(inv) | set(mk) <= set(table) for inv, mk in CTX_WRITES.values())
    assert set(CTX_WRITES) == set(cs.WRITERS) - {"refused", "poison_then_healthy"}
    fallen = set().union(*(set(r["falls"]) for r in table.values()))
    assert not [p for p, r in table.items() if r["parents"] and p not in fallen]
    wrong = []
    for reserved in (False, True):
        for w, (inv, marks) in CTX_WRITES.items():
            s = cs._Seq("x")
            s.base()
            if reserved:
                s.do("reserve", 1)
            s.full()
            assert all(s.m.has(word) for word in CTX_WORD)
            for op, arg in cs._writer_instances(s, w, 0):
                assert s.do(op, arg) is None
            if reserved and "test" in inv:
                inv = inv + CTX_POOL_STACK
            valid = set(table)
            for p in inv:
                valid -= {p} | set(table[p]["falls"])
            for p in marks:
                assert set(table[p]["parents"]) <= valid, (w, p)
                valid.add(p)
            wrong += [(w, reserved, word) for word, p in CTX_WORD.items() if s.m.has(word) != (p in valid)]
    assert not wrong, wrong


def test_the_arena_and_pool_owners_free_each_block_once(tmp_path):
    """csrc/dev_owner.hpp on the counting host allocator of tests/dev_owner_check.cpp: moves, the adoption sequence of an append,
    pool carving and the three growth policies at their boundaries.  The program aborts on a free of a block that is not live
    and fails when a block is live at exit."""
    exe = str(tmp_path / "dev_owner_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc"),
                    os.path.join(ROOT, "tests", "dev_owner_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("case: ") == 8 and run.stdout.rstrip().endswith("all cases passed"), run.stdout


@pytest.fixture(scope="module")
def oracle_run():
    """Every committed sequence on the dense chain, once: [(sequence id, index, call, before, [(ref, tol)])], the conds, the infos."""
    from call_sequences_oracle import Harness
    h, out, conds, failed = Harness(), [], {}, []
    for seq in cs.committed():
        h.start()
        for i, (op, arg) in enumerate(seq["ops"]):
            code, call, pairs, before = h.step(op, arg)
            if op == "fit" and code is None:
                conds[(before.train, before.leaves, tuple(sorted(before.hyper.items())))] = h.oracle.healthy_cond()
                failed.append((before.poisoned, [int(g.info != 0) for g in h.oracle.gps]))
            if pairs is not None:
                out.append((seq["id"], i, call, before, pairs))
    return out, conds, failed


def test_the_references_alone_are_finite_and_well_conditioned(oracle_run):
    """The whole list on the dense float64 chain: every reference value is finite for every healthy leaf and every tolerance is
    finite and positive; cond_2(K_y) of every pool configuration stays below RTOL / eps, where a backward-stable solve's error
    cond eps reaches the north-star relative tolerance the helpers are built on; the poison vector fails exactly the one leaf
    of kernel id 1, and NaN marks exactly its rows."""
    out, conds, failed = oracle_run
    assert len(out) > 1000
    for sid, i, call, before, pairs in out:
        for ref, tol in pairs:
            ref = np.asarray(ref, dtype=np.float64)
            if not before.poisoned:
                assert np.all(np.isfinite(ref)), (sid, i, call)
            else:
                assert np.any(np.isfinite(ref)) or call in ("fit",), (sid, i, call)
            if tol is not None:
                tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
                fin = np.isfinite(ref)
                assert np.all(np.isfinite(tol[fin])), (sid, i, call)
                assert np.all(tol[fin] >= 0) and np.all(tol[fin & (ref != 0)] > 0), (sid, i, call)     # 0: an exact zero (a masked row)
    worst = max(max(c) for c in conds.values())
    print(f"\n{len(out)} reader calls, {len(conds)} pool configurations, largest cond_2(K_y) {worst:.3g}")
    assert worst * EPS <= RTOL, worst
    kid = cs.leaves("S")["kid"]
    for poisoned, info in failed:
        assert info == ([int(k == cs.POISON_KID) for k in kid] if poisoned else [0] * len(info)), (poisoned, info)
    assert any(p for p, _ in failed)


def test_the_oracle_s_kernels_are_the_dense_modules():
    """call_sequences_oracle's gradient rows against targets_grad_dense.column_gradients, and its kernel -- the one table of
    tests/dense_kernels.py -- against itself: the input derivative of every kind against central differences of the value."""
    import call_sequences_oracle as co
    import dense_kernels as dk
    import targets_grad_dense as tgd
    assert co.dk is dk
    Xa, ya = cs.train("A")
    for cls in cs.KIND:
        kind, hyp = cs.hyper(cls, "a", 2)
        g = co.Leaf(kind, hyp, Xa[:60], ya[:60], 0.1)
        Y = np.stack([ya[:60], np.cos(Xa[:60, 0])], axis=1)
        for ard in (False, True):
            G, _, cond = tgd.column_gradients(kind, hyp, Xa[:60], Y, [0.1, 0.2], ard_true=ard)
            assert np.allclose(co.mll_gradients(g, Y, [0.1, 0.2], ard), G, rtol=1e-9, atol=1e-9) and abs(g.cond / cond - 1.0) < 1e-6
    X, _ = cs.train("B")
    A, B = X[:9], X[20:31]
    for cls in cs.KIND:
        kind, hyp = cs.hyper(cls, "b", 5)
        h = hyp[:-1]
        e = 1e-6
        for d in range(5):
            P, M = A.copy(), A.copy()
            P[:, d] += e
            M[:, d] -= e
            fd = (dk.value(kind, h, P, B) - dk.value(kind, h, M, B)) / (2 * e)
            assert np.allclose(dk.d_input(kind, h, A, B)[:, :, d], fd, rtol=1e-6, atol=1e-9)
