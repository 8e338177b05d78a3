"""GPU tests of dsmgp_append_rows: the continued factors against a second context that runs set_train / set_leaves / fit from
scratch on the grown table, and against oracle/gp.py (tests/dense_gp.py for the Matern kind the oracle lacks); the bits the call promises to keep; both storage paths; what can be called
afterwards; state and argument errors; a failed owner; determinism; model.add_data.

Tolerances are the project's: continued against from-scratch factor max|dF| <= 1e-12 max|F|, mll rtol 1e-12, alpha rtol 1e-9 / atol
1e-11 (test_prefix_continue_equals_full_factorisation); against the oracle the RTOL of tests/test_gpu_parity.py; every follow-on
entry point at the tolerance its own GPU test uses against its reference (moment_tol, loo_tol, targets_dense.*_tol, unscaled)."""
import ctypes as C

import numpy as np
import pytest

import append_tables as at
import deepstructuredmixtures_amd as dsm
import dense_gp
import loo_dense
import targets_dense as td
from append_context import grow_by_hand
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd.datagen import regression_data
from oracle import gp as ogp
from pred_tolerance import moment_tol

pytestmark = pytest.mark.gpu

RTOL = 1e-8     # tests/test_gpu_parity.py


def _contexts(n):
    return [hipabi.Context(0) for _ in range(n)]


def _close(*ctxs):
    for c in ctxs:
        c.close()


def _compare_with_scratch(tag, a, b, T, mll_a, info_a, mll_b, info_b):
    """Context a (old fit + append_rows) against context b (from scratch on the grown table): info, mll, factor and alpha of
    every leaf.  Prints every figure before it asserts.  Returns the factors of a."""
    sizes = [len(o) for o in T.grown()[2]]
    return _compare_downloads(tag, at.factors(a, sizes), at.factors(b, sizes), T, mll_a, info_a, mll_b, info_b)


def _compare_downloads(tag, Fa, Fb, T, mll_a, info_a, mll_b, info_b):
    """_compare_with_scratch on factors downloaded already (a context that has moved on since)."""
    sizes = [len(o) for o in T.grown()[2]]
    assert np.array_equal(info_a, info_b), (tag, info_a, info_b)
    for l in range(T.L):
        (F, al), (G, bl) = Fa[l], Fb[l]
        dF, dm = np.max(np.abs(F - G)) / np.max(np.abs(G)), abs(mll_a[l] - mll_b[l]) / abs(mll_b[l])
        print(f"\n{tag} leaf {l} n={sizes[l]}: max|dF|/max|F| {dF:.3g}  mll rel {dm:.3g}  max|dalpha| {np.max(np.abs(al - bl)):.3g}")
        assert dF <= 1e-12, (tag, l, dF)
        assert np.allclose(mll_a[l], mll_b[l], rtol=1e-12, atol=0), (tag, l, mll_a[l], mll_b[l])
        assert np.allclose(al, bl, rtol=1e-9, atol=1e-11), (tag, l, float(np.max(np.abs(al - bl))))
    return Fa


def _oracle(T):
    """(mll, L, alpha) of every leaf of the grown table: oracle/gp.py for the kinds it has (the reference's); tests/dense_gp.py --
    the same leaf in dense SciPy, with the oracle's interface -- for a kind that is not a kernel of the reference (ArdMatern52)."""
    Xg, yg, lists, _, _, mean = T.grown()
    if T.kind_id <= 2:
        k = ogp.make_kernel(T.kind_id, T.hyp[:-1])
        gps = [ogp.GaussianProcess(Xg[o], yg[o], mean[l], k, T.hyp[-1], True).update_cholesky() for l, o in enumerate(lists)]
    else:
        gps = [dense_gp.DenseGP(T.kind_id, T.hyp, Xg[o], yg[o], mean[l]) for l, o in enumerate(lists)]
    assert all(g.info == 0 for g in gps)
    return np.array([g.mll() for g in gps]), [g.L() for g in gps], [np.asarray(g.alpha) for g in gps]


_ORACLE = {}


def _oracle_once(key, T):
    if key not in _ORACLE:
        _ORACLE[key] = _oracle(T)
    return _ORACLE[key]


def _assert_kept_bits(tag, T, before, after, info_old):
    """The leading 128 kb square of every owner (kb = every block of a leaf without additions) is the bits it was."""
    for l, kb in enumerate(T.kept_blocks(info_old)):
        r = min(kb * at.TB, len(T.lists[l]))
        assert r == 0 or np.array_equal(before[l][0][:r, :r], after[l][0][:r, :r]), (tag, l, kb)


# ------------------------------------------------------------------------------------------------ the table

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("fused_steps", [0, 1])
@pytest.mark.parametrize("kind", ["iso", "ard"])
def test_table_against_from_scratch_and_the_oracle(kind, fused_steps, lanes):
    T = at.seven_leaves(kind, "relocate")
    opts = ((hipabi.OPT_FUSED_STEPS, fused_steps), (hipabi.OPT_LANES, lanes))
    a, b = _contexts(2)
    try:
        _, info_old, _ = at.fit_old(a, T, opts)
        assert np.all(info_old == 0)
        before = at.factors(a, [len(o) for o in T.lists])
        mll_a, info_a, sec = at.append(a, T)
        mll_b, info_b, _ = at.fit_grown(b, T, opts)
        assert sec > 0 and np.all(info_a == 0)
        tag = f"{kind} fused_steps={fused_steps} lanes={lanes}"
        after = _compare_with_scratch(tag, a, b, T, mll_a, info_a, mll_b, info_b)
        _assert_kept_bits(tag, T, before, after, info_old)
        assert np.array_equal(before[4][0], after[4][0])                # the leaf without additions: every factor bit
        assert np.array_equal(after[5][0], after[0][0])                 # the COPY pair still shares one factor
        # against the oracle: mll, info (0 everywhere, asserted above and in _oracle), factor and alpha of every leaf at RTOL,
        # relative to the largest entry (cond(K_y) eps is 6e-12 for the IsoSE table and 2e-10 for the Matern one: far inside)
        ref, Lo, ao = _oracle_once(kind, T)
        eL = max(np.max(np.abs(after[l][0] - Lo[l])) / np.max(np.abs(Lo[l])) for l in range(T.L))
        ea = max(np.max(np.abs(after[l][1] - ao[l])) / np.max(np.abs(ao[l])) for l in range(T.L))
        print(f"\n{tag}: against the oracle: max mll rel err {np.max(np.abs(mll_a - ref) / np.abs(ref)):.3g}, "
              f"max|dL|/max|L| {eL:.3g}, max|dalpha|/max|alpha| {ea:.3g}")
        assert np.all(np.abs(mll_a - ref) <= RTOL * np.abs(ref))
        assert eL <= RTOL and ea <= RTOL
        st = a.append_stats()
        print(f"\n{tag}: {st}")
        # owners continued: 0, 1, 3, 6; restarted: 2; one block column each for 0, 1, 2, 3, 6; npad of leaf 1 grew: relocation
        assert st == dict(owners_continued=4, leaves_untouched=0, bytes_relocated=st["bytes_relocated"], block_columns_factorised=5,
                          owners_restarted=1, copies_dissolved=0)
        # kept squares of leaves 0, 1, 3, 4, 6: 2, 1, 5, 2 (leaf 4: 200 rows = 2 block rows, all kept) and 2 blocks wide, with as
        # many Dinv blocks each
        tiles = (2 * 2 + 2) + (1 + 1) + (5 * 5 + 5) + (2 * 2 + 2) + (2 * 2 + 2)
        assert st["bytes_relocated"] == tiles * 128 * 128 * 8
        # the call is described as a fit would be
        tm, (flops, launches) = a.timings(), a.work()
        assert abs(tm["total_fit"] - sec) <= 1e-12 and launches > 0
        full_flops = b.work()[0]
        print(f"\n{tag}: update flops of the call {flops:.4g}, of the from-scratch fit {full_flops:.4g}")
        assert 0 < flops < full_flops
    finally:
        _close(a, b)


# ------------------------------------------------------------------------------------------------ in place and split

def test_in_place_when_no_padded_size_changes():
    T = at.seven_leaves("iso", "in_place")
    a, b = _contexts(2)
    try:
        _, info_old, _ = at.fit_old(a, T)
        before = at.factors(a, [len(o) for o in T.lists])
        mll_a, info_a, _ = at.append(a, T)
        mll_b, info_b, _ = at.fit_grown(b, T)
        after = _compare_with_scratch("in place", a, b, T, mll_a, info_a, mll_b, info_b)
        _assert_kept_bits("in place", T, before, after, info_old)
        st = a.append_stats()
        print(f"\nin place: {st}")
        assert st["bytes_relocated"] == 0
        assert st == dict(owners_continued=3, leaves_untouched=2, bytes_relocated=0, block_columns_factorised=4, owners_restarted=1,
                          copies_dissolved=0)
        for l in (1, 4):                                                # no additions, same mean: every factor bit
            assert np.array_equal(before[l][0], after[l][0])
    finally:
        _close(a, b)


def test_copy_pair_with_different_additions_dissolves():
    T = at.seven_leaves("iso", "split")
    a, b = _contexts(2)
    try:
        _, info_old, _ = at.fit_old(a, T)
        before = at.factors(a, [len(o) for o in T.lists])
        mll_a, info_a, _ = at.append(a, T)
        mll_b, info_b, _ = at.fit_grown(b, T)
        after = _compare_with_scratch("split", a, b, T, mll_a, info_a, mll_b, info_b)
        _assert_kept_bits("split", T, before, after, info_old)
        st = a.append_stats()
        print(f"\nsplit: {st}")
        assert st["copies_dissolved"] == 1 and st["owners_continued"] == 5 and st["bytes_relocated"] > 0
        assert after[5][0].shape == (319, 319) and after[0][0].shape == (320, 320)
        assert np.array_equal(after[5][0][:256, :256], before[0][0][:256, :256])       # continued from the source's old factor
    finally:
        _close(a, b)


@pytest.mark.parametrize("variant", ["in_place", "relocate"])
def test_many_small_leaves_through_fused_steps(variant):
    T = at.many_small_leaves(variant)
    a, b = _contexts(2)
    try:
        _, info_old, _ = at.fit_old(a, T)
        assert a.work_fused()[1] > 0                                    # the old fit did run fused steps
        before = at.factors(a, [len(o) for o in T.lists])
        mll_a, info_a, _ = at.append(a, T)
        if variant == "relocate":       # (in place the continuation is block (1, 1) alone: a fused step of diagonal-block tasks,
            assert a.work_fused()[1] > 0        # which the count of fused TILE launches does not see)
        mll_b, info_b, _ = at.fit_grown(b, T)
        after = _compare_with_scratch(f"small leaves {variant}", a, b, T, mll_a, info_a, mll_b, info_b)
        _assert_kept_bits(variant, T, before, after, info_old)
        assert np.array_equal(before[39][0], after[39][0])
        st = a.append_stats()
        print(f"\nsmall leaves {variant}: {st}")
        assert (st["bytes_relocated"] == 0) == (variant == "in_place")
        assert st["owners_continued"] == 39 and st["owners_restarted"] == 0
        assert st["leaves_untouched"] == (1 if variant == "in_place" else 0)
    finally:
        _close(a, b)


# ------------------------------------------------------------------------------------------------ after the call

def _check(tag, got, ref, tol):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    err = np.abs(got - ref)
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(err / tol):.3g}")
    assert np.all(err <= tol), tag


def test_entry_points_after_the_call():
    """a: old fit + append_rows; b: from scratch on the grown table.  Every follow-on entry point of a against b."""
    T = at.seven_leaves("iso", "relocate")
    Xg, yg, lists, _, _, mean = T.grown()
    noise = float(np.exp(2.0 * T.hyp[-1]))                  # (lib_noise of tests/test_loo_gpu.py)
    rng = np.random.default_rng(3)
    nt = 40
    Xt = np.asfortranarray(rng.uniform(size=(nt, 2)))
    rptr, ridx = np.arange(T.L + 1) * nt, np.tile(np.arange(nt), T.L)
    a, b = _contexts(2)
    try:
        at.fit_old(a, T)
        a.set_test(Xt, rptr, ridx)                                      # a resident test set, targets and L^-T: they fall with the call
        a.predict_run()
        a.loo()
        a.solve_targets(np.stack([T.y, -T.y], axis=1))
        at.append(a, T)
        at.fit_grown(b, T)
        with pytest.raises(hipabi.DsmgpError) as e:
            a.predict_run()
        assert e.value.code == hipabi.E_STATE
        with pytest.raises(hipabi.DsmgpError) as e:
            a.predict_targets()
        assert e.value.code == hipabi.E_STATE
        yscale = max(1.0, float(np.max(np.abs(yg))))
        res = []
        for c in (a, b):
            c.set_test(Xt, rptr, ridx)
            c.predict_run()
            res.append(c.predict_fetch())
        tm, tv = moment_tol(res[1][0], res[1][1], np.ones(T.L * nt), noise, yscale)
        _check("predict mu", res[0][0], res[1][0], tm)
        _check("predict var", res[0][1], res[1][1], tv)
        ga, gb = a.gradients(3), b.gradients(3)
        _check("gradients", ga, gb, 1e-9 * max(1.0, float(np.max(np.abs(gb)))))
        (ma, va, la), (mb, vb, lb) = a.loo(), b.loo()
        ptr = np.concatenate([[0], np.cumsum([len(o) for o in lists])])
        for l, o in enumerate(lists):
            s = slice(ptr[l], ptr[l + 1])
            tmu, tvar, _, ts = loo_dense.loo_tol(yg[o], mb[s], vb[s], np.ones(len(o)), noise)
            _check(f"loo mu leaf {l}", ma[s], mb[s], tmu)
            _check(f"loo var leaf {l}", va[s], vb[s], tvar)
            _check(f"loo lpd leaf {l}", la[l], lb[l], ts)
        Y = np.stack([yg, np.cos(5.0 * Xg[:, 0])], axis=1)
        M = np.stack([mean, np.zeros(T.L)], axis=1)
        (ta, _), (tb, _) = a.solve_targets(Y, M), b.solve_targets(Y, M)
        for l, o in enumerate(lists):
            F, _ = b.download_factor(l, len(o))
            cond = float(np.linalg.cond(F)) ** 2
            Z = b.targets_fetch(l)
            _check(f"targets mll leaf {l}", ta[l], tb[l], td.mll_tol(Z, F, cond))
            _check(f"targets Z leaf {l}", a.targets_fetch(l), Z, td.z_tol(Z, cond))
        mua, mub = a.predict_targets(), b.predict_targets()
        _check("targets mu", mua, mub, td.mu_tol(mub, Y))
        # set_hyper + fit: a plain full fit under the schedule the call left (COPY where kept, FULL elsewhere) -- the same plan
        # as b's, so the same launches and the same bits: nothing of the one-shot continuation is left in the phase lists
        hyp2 = T.hyp + np.array([0.1, -0.05, 0.02])
        out = []
        for c in (a, b):
            c.set_hyper(0, T.kind_id, hyp2)
            mll, info, _ = c.fit()
            out.append((mll, info, at.factors(c, [len(o) for o in lists]), c.work(), c.work_fused()))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        assert out[0][3] == out[1][3] and out[0][4] == out[1][4]
        for (Fa, ala), (Fb, alb) in zip(out[0][2], out[1][2]):
            assert np.array_equal(Fa, Fb) and np.array_equal(ala, alb)
    finally:
        _close(a, b)


def test_a_second_call_on_top_of_the_first():
    T = at.seven_leaves("iso", "relocate")
    Xg, yg, lists, op, src, mean = T.grown()
    rng = np.random.default_rng(11)
    Xn2 = np.asfortranarray(rng.uniform(size=(8, 2)))
    yn2 = np.sin(3.0 * Xn2[:, 0]) + 0.5
    adds2 = [np.arange(0, 8), np.zeros(0, np.int64), np.array([1, 5]), np.arange(2, 6), np.array([7]), np.arange(0, 8), np.array([0])]
    T2 = at.Table("iso", Xg, yg, lists, op, src, [0] * T.L, mean, Xn2, yn2, adds2, None)
    a, b = _contexts(2)
    try:
        at.fit_old(a, T)
        at.append(a, T)
        before = at.factors(a, [len(o) for o in lists])
        mll_a, info_a, _ = at.append(a, T2)
        mll_b, info_b, _ = at.fit_grown(b, T2)
        after = _compare_with_scratch("second call", a, b, T2, mll_a, info_a, mll_b, info_b)
        _assert_kept_bits("second call", T2, before, after, None)
        st = a.append_stats()
        print(f"\nsecond call: {st}")
        assert st["bytes_relocated"] == 0 and st["leaves_untouched"] == 1 and st["copies_dissolved"] == 0
    finally:
        _close(a, b)


# ------------------------------------------------------------------------------------------------ state and arguments

def test_state_errors():
    T = at.seven_leaves("iso", "in_place")
    (a,) = _contexts(1)
    try:
        ptr, idx = T.add_csr()
        a.set_train(T.X, T.y)
        a.set_leaves(*at._csr(T.lists), T.kid, T.mean)
        a.set_hyper(0, T.kind_id, T.hyp)
        with pytest.raises(hipabi.DsmgpError) as e:                     # before the first fit
            a.append_rows(T.Xn, T.yn, ptr, idx)
        assert e.value.code == hipabi.E_STATE
        at.fit_old(a, T)
        a.set_hyper(0, T.kind_id, T.hyp + 0.01)
        with pytest.raises(hipabi.DsmgpError) as e:                     # the fit is not current
            a.append_rows(T.Xn, T.yn, ptr, idx)
        assert e.value.code == hipabi.E_STATE
        with pytest.raises(hipabi.DsmgpError) as e:
            a.append_stats()                                            # no call has succeeded yet
        assert e.value.code == hipabi.E_STATE
        a.reserve(256 << 20)
        at.fit_old(a, T)
        with pytest.raises(hipabi.DsmgpError) as e:                     # under a reserved pool
            a.append_rows(T.Xn, T.yn, ptr, idx)
        assert e.value.code == hipabi.E_STATE
        a.reserve(0)
        at.fit_old(a, T)
        at.append(a, T)                                                 # and the context is usable afterwards
        assert a.append_stats()["bytes_relocated"] == 0
    finally:
        _close(a)


def test_argument_errors_leave_the_context_as_it_was():
    T = at.seven_leaves("iso", "relocate")
    a, b = _contexts(2)
    try:
        at.fit_old(a, T)
        sizes = [len(o) for o in T.lists]
        before, tm, work = at.factors(a, sizes), a.timings(), a.work()
        ptr, idx = T.add_csr()
        m = T.Xn.shape[0]

        def raw(X=T.Xn, y=T.yn, m_=m, D=2, p=ptr, i=idx, mean=None):
            """The C entry point itself: what the Python wrapper would refuse before it gets there."""
            as_d = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)       # noqa: E731
            as_l = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.int64)         # noqa: E731
            X, y, p, i, mean = (None if X is None else np.asfortranarray(X, dtype=np.float64)), as_d(y), as_l(p), as_l(i), as_d(mean)
            ptr_of = lambda v, t: None if v is None else v.ctypes.data_as(t)                        # noqa: E731
            dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
            return a.lib.dsmgp_append_rows(a.h, ptr_of(X, dp), ptr_of(y, dp), m_, D, ptr_of(p, lp), ptr_of(i, lp), ptr_of(mean, dp),
                                           None, None, None)

        def bad(v, at_, val):
            v = np.array(v, dtype=np.float64 if np.asarray(v).dtype.kind == "f" else np.int64, copy=True, order="K")
            v[at_] = val
            return v

        big = (1 << 20) - 299                                           # leaf 0 has 300 rows: one more than the limit allows
        bigptr = np.concatenate([[0], np.full(T.L, big)])
        cases = {
            "m < 1": dict(m_=0),
            "another D": dict(D=3),
            "X_new NULL": dict(X=None), "y_new NULL": dict(y=None), "add_ptr NULL": dict(p=None), "add_idx NULL": dict(i=None),
            "non-finite X_new": dict(X=bad(T.Xn, (7, 1), np.nan)), "non-finite y_new": dict(y=bad(T.yn, 3, np.inf)),
            "non-finite mean": dict(mean=bad(T.mean, 2, np.nan)),
            "add_ptr[0] != 0": dict(p=bad(ptr, 0, 1)),
            "position outside 0..m-1": dict(i=bad(idx, 5, m)), "negative position": dict(i=bad(idx, 5, -1)),
            "not strictly ascending": dict(i=bad(idx, 6, idx[5])),
            "leaf beyond the size limit": dict(X=np.zeros((big, 2)), y=np.zeros(big), m_=big, p=bigptr, i=np.arange(big)),
        }
        for name, kw in cases.items():
            assert raw(**kw) == hipabi.E_ARG, name
            after = at.factors(a, sizes)
            for (F, al), (G, bl) in zip(before, after):
                assert np.array_equal(F, G) and np.array_equal(al, bl), name
            assert a.timings() == tm and a.work() == work, name
        mll_a, info_a, _ = at.append(a, T)                              # the same context then takes the valid call
        mll_b, info_b, _ = at.fit_grown(b, T)
        _compare_with_scratch("after the refusals", a, b, T, mll_a, info_a, mll_b, info_b)
    finally:
        _close(a, b)


# ------------------------------------------------------------------------------------------------ a failed owner

def _run_failed_owner(c, with_it):
    X, y, Xn, yn, lists, adds, kid, mean = at.failed_owner_table(with_it)
    c.set_train(X, y)
    c.set_leaves(*at._csr(lists), kid, mean)
    for k, (kind, hyp) in at.FAILED_HYP.items():
        c.set_hyper(k, kind, hyp)
    _, info_old, _ = c.fit()
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in adds])])
    mll, info, _ = c.append_rows(Xn, yn, ptr, np.concatenate(adds))
    sizes = [len(o) + len(x) for o, x in zip(lists, adds)]
    return info_old, mll, info, at.factors(c, sizes), c.append_stats()


def test_failed_owner_restarts_and_disturbs_nobody():
    import scipy.linalg as sla
    X, y, Xn, yn, lists, adds, _, _ = at.failed_owner_table()
    Xg = np.vstack([X, Xn])
    rows = np.concatenate([lists[0], X.shape[0] + adds[0]])
    K = Xg[rows] @ Xg[rows].T + (np.exp(-60.0) + 1e-8) * np.eye(rows.size)
    _, linfo = sla.lapack.dpotrf(K, lower=1)
    assert linfo == 4
    a, b = _contexts(2)
    try:
        info_old, mll, info, Fa, st = _run_failed_owner(a, True)
        assert info_old[0] == 4 and np.all(info_old[1:] == 0)
        assert info[0] == linfo and np.all(info[1:] == 0)
        print(f"\nfailed owner: {st}")
        assert st["owners_restarted"] == 1 and st["owners_continued"] == 3
        assert st["block_columns_factorised"] == 2 + 1 + 1 + 1            # the failed leaf: both of its block columns
        _, mll_b, info_b, Fb, st_b = _run_failed_owner(b, False)          # the same run without it
        assert st_b["owners_restarted"] == 0 and st_b["owners_continued"] == 3
        assert np.array_equal(mll[1:], mll_b) and np.array_equal(info[1:], info_b)
        for (F, al), (G, bl) in zip(Fa[1:], Fb):
            assert np.array_equal(F, G) and np.array_equal(al, bl)
    finally:
        _close(a, b)


def test_first_bad_minor_inside_the_new_blocks_has_its_absolute_order():
    """An owner whose old fit was fine (info 0) and whose NEW rows make the matrix singular: the recipe of
    test_first_bad_minor_is_reported_exactly -- IsoLinear, l = 1, rows 2^27 e_i, noise and jitter absorbed by rounding, every
    operation exact.  130 orthogonal old rows (K_y = 2^54 I: positive definite, kb = 1 kept block); the second appended row repeats
    old row 5, so its pivot is exactly 0: the first bad leading minor has order 130 + 2 = 132, inside block column 1, which the
    continuation factorises -- in LAPACK on the grown matrix, in a from-scratch context and in the continued one.  D = 140 > 32:
    the Gram tiles go through memory, the path on which a continuing leaf's Gram list starts at its first new block row; the
    padded size stays 256, so the call runs in place."""
    import scipy.linalg as sla
    D, n0 = 140, 130
    X = np.zeros((n0, D))
    X[np.arange(n0), np.arange(n0)] = 2.0 ** 27
    Xn = np.zeros((4, D))
    Xn[0, 130], Xn[1, 5], Xn[2, 131], Xn[3, 132] = (2.0 ** 27,) * 4
    Xg = np.vstack([X, Xn])
    K = Xg @ Xg.T + (np.exp(-60.0) + 1e-8) * np.eye(n0 + 4)
    assert K[0, 0] == 2.0 ** 54                                        # the shift is absorbed
    assert sla.lapack.dpotrf(K[:n0, :n0].copy(), lower=1)[1] == 0
    linfo = sla.lapack.dpotrf(K, lower=1)[1]
    assert linfo == 132
    a, b = _contexts(2)
    try:
        a.set_train(X, np.zeros(n0))
        a.set_leaves([0, n0], np.arange(n0), [0], [0.0])
        a.set_hyper(0, 2, [0.0, 0.0, -30.0])
        _, info_old, _ = a.fit()
        assert info_old[0] == 0
        F_old, _ = a.download_factor(0, n0)
        _, info, _ = a.append_rows(Xn, np.zeros(4), [0, 4], np.arange(4))
        st = a.append_stats()
        print(f"\nbad minor in the new blocks: info {int(info[0])}, LAPACK {linfo}, {st}")
        assert info[0] == linfo
        assert st["owners_continued"] == 1 and st["owners_restarted"] == 0 and st["bytes_relocated"] == 0
        F_new, _ = a.download_factor(0, n0 + 4)
        assert np.array_equal(F_new[:128, :128], F_old[:128, :128])    # the kept block is the bits it was
        b.set_train(Xg, np.zeros(n0 + 4))
        b.set_leaves([0, n0 + 4], np.arange(n0 + 4), [0], [0.0])
        b.set_hyper(0, 2, [0.0, 0.0, -30.0])
        _, info_b, _ = b.fit()
        assert info_b[0] == linfo
        # the next call finds a failed owner and restarts it from block 0: the same first bad minor
        _, info2, _ = a.append_rows(Xn[2:3] * 0.5, np.zeros(1), [0, 1], [0])
        assert info2[0] == linfo and a.append_stats()["owners_restarted"] == 1
    finally:
        _close(a, b)


# ------------------------------------------------------------------------------------------------ determinism, model level

def test_two_contexts_through_the_same_sequence_agree_bitwise():
    T = at.seven_leaves("iso", "relocate")
    out = []
    ctxs = _contexts(2)
    try:
        for c in ctxs:
            at.fit_old(c, T)
            mll, info, _ = at.append(c, T)
            out.append((mll, info, at.factors(c, [len(o) for o in T.grown()[2]]), c.append_stats()))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][3] == out[1][3]
        for (F, al), (G, bl) in zip(out[0][2], out[1][2]):
            assert np.array_equal(F, G) and np.array_equal(al, bl)
    finally:
        _close(*ctxs)


def _transition_tables():
    """Leaves of 100, 130 and 260 rows (padded 128, 256, 384: the smallest table in which an appended row can and cannot move a
    padded size) and a COPY of the 260-row leaf; D = 2.  T1 adds rows that leave every padded size as it is; T2, on top of it,
    takes the 100-row leaf (110 by then) past 128 and gives the 130-row leaf nothing.  24 routed test rows."""
    X, y, Xn1, yn1 = at._data("iso", 490, 23, 4711)
    _, _, Xn2, yn2 = at._data("iso", 1, 28, 4712)
    lists = [np.arange(0, 100), np.arange(100, 230), np.arange(230, 490), np.arange(230, 490)]
    op, src = [at.SHARE_FULL] * 3 + [at.SHARE_COPY], [-1, -1, -1, 2]
    mean = [0.5, 0.4, 0.6, 0.45]
    adds1 = [np.arange(0, 10), np.arange(10, 15), np.arange(15, 23), np.arange(15, 23)]
    T1 = at.Table("iso", X, y, lists, op, src, [0] * 4, mean, Xn1, yn1, adds1, None)
    Xg, yg, lists1, op1, src1, mean1 = T1.grown()
    adds2 = [np.arange(0, 25), np.zeros(0, np.int64), np.arange(25, 28), np.arange(25, 28)]
    T2 = at.Table("iso", Xg, yg, lists1, op1, src1, [0] * 4, mean1, Xn2, yn2, adds2, [0.52, 0.4, 0.61, 0.44])
    assert [-(-len(o) // at.TB) for o in lists] == [-(-len(o) // at.TB) for o in lists1] == [1, 2, 3, 3]
    assert [-(-len(o) // at.TB) for o in T2.grown()[2]] == [2, 2, 3, 3] and T2.grown()[3] == op
    c = [10, 6, 5, 3]
    Xt = np.asfortranarray(np.random.default_rng(8).uniform(size=(max(c), 2)))
    rptr = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
    assert rptr[-1] == 24
    return T1, T2, (Xt, rptr, np.concatenate([np.arange(k) for k in c]).astype(np.int64), c)


def _walk_the_transitions(a, T1, T2, test):
    """The sequence of test_one_context_through_every_ownership_transition on context a.  Returns every output in order and,
    per append, what the comparison with a fresh context needs."""
    Xt, rptr, ridx, c = test
    out, calls = [], []

    def registered_and_predicted():
        a.set_test(Xt, rptr, ridx)
        a.predict_run()
        out.extend(a.predict_fetch())

    out.extend(at.fit_old(a, T1)[:2])
    registered_and_predicted()
    out.append(a.gradients(3))
    for pool in (256 << 20, 0):                                         # every arena carved from the pool, then its own again
        a.reserve(pool)
        out.extend(a.fit()[:2])
        registered_and_predicted()
    for T in (T1, T2):
        n_old, n_new = [len(o) for o in T.lists], [len(o) for o in T.grown()[2]]
        before = at.factors(a, n_old)
        V0 = [a.download_vt(l, c[l], n_old[l]) for l in range(T.L)]
        ptr, idx = T.add_csr()
        mll, info, _ = a.append_rows(T.Xn, T.yn, ptr, idx, T.mean_new, keep_test=True)
        a.predict_run()
        mu, var = a.predict_fetch()
        after = at.factors(a, n_new)
        V1 = [a.download_vt(l, c[l], n_new[l]) for l in range(T.L)]
        calls.append(dict(mll=mll, info=info, before=before, after=after, V0=V0, V1=V1, mu=mu, var=var,
                          append_stats=a.append_stats(), resume_stats=a.resume_stats()))
        out.extend([mll, info, mu, var] + [x for F, al in after for x in (F, al)] + V1)
    grads = a.gradients(3)
    loo = a.loo()
    out.extend([grads, *loo])
    return out, calls, grads, loo


def test_one_context_through_every_ownership_transition():
    """fit, set_test, predict_run, gradients; the same under a reserved pool and again without it; an append that keeps the test
    set in place, predict_run; one that relocates, predict_run, gradients, loo.  After each append a fresh context b on the grown
    table: factors, mll and alpha as test_table_against_from_scratch_and_the_oracle compares them, the moments within
    pred_tolerance.moment_tol; the kept blocks and the kept columns of K_tn L^-T are the bits a had before the call.  A second
    context through the same sequence gives the same bits everywhere."""
    T1, T2, test = _transition_tables()
    Xt, rptr, ridx, c = test
    a, a2 = _contexts(2)
    try:
        out, calls, grads, loo = _walk_the_transitions(a, T1, T2, test)
        out2 = _walk_the_transitions(a2, T1, T2, test)[0]
        assert len(out) == len(out2)
        for i, (x, y) in enumerate(zip(out, out2)):
            assert np.array_equal(x, y), f"output {i} of the two contexts differs"
        for T, r, tag in ((T1, calls[0], "transitions: in place"), (T2, calls[1], "transitions: relocate")):
            Xg, yg, lists, _, _, mean = T.grown()
            (b,) = _contexts(1)
            try:
                mll_b, info_b, _ = at.fit_grown(b, T)
                assert np.all(r["info"] == 0)
                sizes = [len(o) for o in lists]
                _compare_downloads(tag, r["after"], at.factors(b, sizes), T, r["mll"], r["info"], mll_b, info_b)
                ref, Lo, ao = _oracle(T)
                assert np.all(np.abs(r["mll"] - ref) <= RTOL * np.abs(ref)), tag
                assert max(np.max(np.abs(r["after"][l][0] - Lo[l])) / np.max(np.abs(Lo[l])) for l in range(T.L)) <= RTOL, tag
                assert max(np.max(np.abs(r["after"][l][1] - ao[l])) / np.max(np.abs(ao[l])) for l in range(T.L)) <= RTOL, tag
                b.set_test(Xt, rptr, ridx)
                b.predict_run()
                mb, vb = b.predict_fetch()
                noise = float(np.exp(2.0 * T.hyp[-1]))
                tm, tv = moment_tol(mb, vb, np.ones(mb.size), noise, max(1.0, float(np.max(np.abs(yg)))))
                _check(f"{tag} mu", r["mu"], mb, tm)
                _check(f"{tag} var", r["var"], vb, tv)
                if T is T2:
                    gb = b.gradients(3)
                    _check(f"{tag} gradients", grads, gb, 1e-9 * max(1.0, float(np.max(np.abs(gb)))))
                    mlb, vlb, llb = b.loo()
                    ptr = np.concatenate([[0], np.cumsum(sizes)])
                    for l, o in enumerate(lists):
                        s = slice(ptr[l], ptr[l + 1])
                        tmu, tvar, _, ts = loo_dense.loo_tol(yg[o], mlb[s], vlb[s], np.ones(len(o)), noise)
                        _check(f"{tag} loo mu leaf {l}", loo[0][s], mlb[s], tmu)
                        _check(f"{tag} loo var leaf {l}", loo[1][s], vlb[s], tvar)
                        _check(f"{tag} loo lpd leaf {l}", loo[2][l], llb[l], ts)
            finally:
                _close(b)
            _assert_kept_bits(tag, T, r["before"], r["after"], None)
            kb = T.kept_blocks(None)
            for l in range(T.L):                                        # a COPY leaf reads its source's factor
                k = min((kb[T.src[l]] if T.op[l] == at.SHARE_COPY else kb[l]) * at.TB, len(T.lists[l]))
                assert k == 0 or np.array_equal(r["V0"][l][:, :k], r["V1"][l][:, :k]), (tag, l, k)
            print(f"\n{tag}: {r['append_stats']} {r['resume_stats']}")
            assert r["resume_stats"]["test_set_dropped"] == 0 and r["resume_stats"]["leaves_kept"] > 0
        assert calls[0]["append_stats"]["bytes_relocated"] == 0 and calls[0]["resume_stats"]["bytes_relocated"] == 0
        assert calls[1]["append_stats"]["bytes_relocated"] > 0 and calls[1]["resume_stats"]["bytes_relocated"] > 0
    finally:
        _close(a, a2)


def test_add_data_on_a_small_dsmgp_against_the_hand_grown_copy():
    N, D = 3000, 3
    X, y, Xt = regression_data(N, D, n_test=200, seed=900)
    Xn, yn, _ = regression_data(40, D, n_test=1, seed=901)
    kw = dict(M=60, kernel=dsm.IsoSE(np.log(0.3), 0.0), logNoise=np.log(0.1), seed=4)
    m, h = dsm.buildDSMGP(X, y, 3, 4, **kw), dsm.buildDSMGP(X, y, 3, 4, **kw)
    try:
        sec = dsm.add_data(m, Xn, yn)
        print(f"\nadd_data: {float(sec):.4g} s, {sec.stats}")
        assert sec > 0 and sec.fallback is False and sec.stats["owners_continued"] + sec.stats["owners_restarted"] > 0
        grow_by_hand("dsmgp", h, Xn, yn)
        assert all(np.array_equal(p.obs, q.obs) and p.mean.m == q.mean.m for p, q in zip(m.leaves, h.leaves))
        err = np.abs(m.leaf_mll - h.leaf_mll) / np.abs(h.leaf_mll)
        print(f"\nadd_data: max leaf mll rel err {np.max(err):.3g}")
        assert np.allclose(m.leaf_mll, h.leaf_mll, rtol=RTOL, atol=1e-8) and np.array_equal(m.leaf_info, h.leaf_info)
        za, zb = dsm.update(m), dsm.update(h)
        assert abs(za - zb) <= RTOL * max(1.0, abs(zb))
        (mu, var), (mo, vo) = dsm.predict(m, Xt), dsm.predict(h, Xt)
        assert np.allclose(mu, mo, rtol=RTOL, atol=1e-9) and np.allclose(var, vo, rtol=RTOL, atol=1e-9)
        t0 = dsm.fit(m, 0.05)                                           # the follow-up fit: a plain full fit of the grown table
        assert t0 > 0 and np.allclose(m.leaf_mll, h.leaf_mll, rtol=RTOL, atol=1e-8)
    finally:
        m.ctx.close()
        h.ctx.close()
