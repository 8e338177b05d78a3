"""GPU tests of dsmgp_predict_columns_gradients: the gradients of the predictive means of every target column of every (leaf,
routed row) entry with respect to the test point (targets_inputgrad_kernel, targets_inputgrad_finish_kernel).

Reference of column 0 of the single-leaf cases: tests/golden/gp_predgrad.npz (50 digits) within predgrad_dense.tolerances; the
other columns, the leaf table and the larger single GP are compared with the dense float64 helper
tests/targets_inputgrad_dense.py fed with download_factor of the same context, within twice that tolerance because both sides
carry float64 rounding (the rule of tests/test_predgrad_gpu.py).  The exact properties are checked on bits."""
import ctypes as C
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import datagen, hipabi
import dense_kernels as dk
import predgrad_dense as pgd
import targets_inputgrad_dense as tid
from test_predcov_gpu import TABLE, _same_bits, _table_setup

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_predgrad.npz"))
CASE_NAMES = sorted(k[:-5] for k in Z.files if k.endswith("/meta"))
KIND_NAMES = ["isose", "ardse", "isolinear", "ardlinear", "ardseproduct", "isomatern32", "isomatern52", "ardmatern32", "ardmatern52"]
RQ_NAMES = [n for n in CASE_NAMES if int(Z[n + "/meta"][0]) in dk.RQ]
FAR = 1e3


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _columns(c, Q, seed):
    """(Y, mean): column 0 is the case's y with its mean, the others come from the counter stream of datagen."""
    X, n = c["X"], c["X"].shape[0]
    Y = np.empty((n, Q), order="F")
    Y[:, 0] = c["y"]
    for j in range(1, Q):
        Y[:, j] = (1.0 + 0.5 * j) * np.sin((1.0 + j % 5) * X[:, 0]) + 3.0 * (j % 3) + 0.1 * datagen.normal(seed + j, 0, n)
    mean = np.mean(Y, axis=0) + 0.25
    mean[0] = c["mean"]
    return Y, mean


def loghyp_of(kind, D):
    """The library's hyper-vector without the noise (the rule of tests/test_predgrad_gpu.py; alpha = 1.5 for the RQ kinds)."""
    ls = np.array([0.35, 0.5, 0.42])[:D] * np.sqrt(D) if D <= 3 else np.full(D, 0.3 * np.sqrt(D))
    if kind in dk.LINEAR:
        ls = ls + 0.5
    return dk.pack(kind, np.log(ls[:D if kind in dk.ARD else 1]), 0.0 if kind in dk.LINEAR else 0.1, loga=np.log(1.5))


def make_case(kind, n, nt, D, seed):
    X = datagen.uniform(seed, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * datagen.normal(seed + 1, 0, n) + 0.7
    Xt = datagen.uniform(seed + 2, 0, nt * D).reshape((nt, D), order="F") * 1.2 - 0.1
    Xt[0] = X[n - 1]                                # a test row AT a training row
    far = []
    if kind not in dk.LINEAR and kind not in dk.RQ:
        Xt[2], Xt[3] = FAR, -FAR
        far = [2, 3]
    Xt[4] = Xt[1]                                   # one row listed twice, in one 128-row tile
    return dict(kind=kind, X=np.asfortranarray(X), y=y, Xt=np.asfortranarray(Xt), mean=float(np.mean(y)) + 0.25,
                loghyp=loghyp_of(kind, D), logNoise=float(np.log(0.1)), far=far, dup=(1, 4))


def _single(ctx, c, path):
    X, y, Xt = c["X"], c["y"], c["Xt"]
    n, nt = X.shape[0], Xt.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
    ctx.set_hyper(0, c["kind"], np.concatenate([c["loghyp"], [c["logNoise"]]]))
    if path == "joint":
        ctx.set_test(Xt, [0, nt], np.arange(nt))
        _, info, _ = ctx.fit()
        ctx.predict_run()
    else:
        _, info, _ = ctx.fit()
        ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
    assert info[0] == 0


def _dense(ctx, leaf, c, Y, mean):
    """(dmu, tolerance) of the dense helper on the device's own factor."""
    F, _ = ctx.download_factor(leaf, c["X"].shape[0])
    ref = tid.moments(c["kind"], c["loghyp"], c["logNoise"], c["X"], Y, mean, c["Xt"], L=np.tril(F))[2]
    return ref, tid.tolerances(c["kind"], c["loghyp"], c["logNoise"], c["X"], Y, c["Xt"], ref)


def _check(tag, got, ref, tol):
    err = np.abs(got - ref)
    ratio = err / tol
    print(f"\n{tag}: max err {np.max(err):.3g}, worst err/tol {np.max(ratio):.3g}")
    w = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    assert np.all(err <= tol), (tag, w, got[w], ref[w], tol[w])


def _check_case(ctx, c, path, tag, golden=True):
    _single(ctx, c, path)
    nt, D = c["Xt"].shape
    Y, mean = _columns(c, 3, 9100)
    ctx.solve_targets(Y, mean[None, :])
    dmu = ctx.predict_targets_gradients()
    assert dmu.shape == (nt, D, 3) and dmu.flags.f_contiguous and ctx.predict_targets_gradients_seconds > 0.0
    ref, tol = _dense(ctx, 0, c, Y, mean)
    if golden:
        t0 = pgd.tolerances(c["kind"], c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], c["dmu"], c["dvar"])[0]
        _check(tag + " column 0 against 50 digits", dmu[:, :, 0], c["dmu"], t0)
    else:
        _check(tag + " column 0", dmu[:, :, 0], ref[:, :, 0], 2.0 * tol[:, :, 0])
    _check(tag + " columns 1, 2", dmu[:, :, 1:], ref[:, :, 1:], 2.0 * tol[:, :, 1:])
    # exact properties, on bits
    assert _same_bits(dmu, ctx.predict_targets_gradients())
    a, b = c["dup"]
    assert _same_bits(dmu[a], dmu[b])
    for p in c["far"]:
        assert np.all(dmu[p] == 0.0), (tag, p, dmu[p])
    ctx.solve_targets(Y[:, 1], mean[None, 1:2])                     # a column solved alone
    assert _same_bits(ctx.predict_targets_gradients()[:, :, 0], dmu[:, :, 1])
    ctx.solve_targets(c["y"], np.array([[c["mean"]]]))              # Q = 1, Y = y: dsmgp_predict_gradients' dmu, another kernel
    one = ctx.predict_targets_gradients()[:, :, 0]
    assert _same_bits(one, dmu[:, :, 0])
    single = ctx.predict_gradients(want_var=False)[0]
    t1 = pgd.tolerances(c["kind"], c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], single, np.zeros_like(single))[0]
    _check(tag + " Q = 1 against predict_gradients", one, single, 2.0 * t1)


@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("kind", range(9))
def test_fixture_cases_against_50_digits(ctx, kind, path):
    """Every fixture case of the kind (five shapes, D = 1 and 3; D = 40 for IsoSE and ArdSEProduct, whose 40 length-scales are
    EQUAL, so those two cases cannot tell one dimension's factor from another's) on both routes to K_tn L^-T: column 0 against
    the 50 digits within the tolerance, the other columns against the dense helper within twice it; then the exact properties on
    bits.  Every kind, the rational quadratic ones included, past D = 8 with distinct length-scales: tests/test_wide_inputs_gpu.py."""
    names = [n for n in CASE_NAMES if n.startswith(KIND_NAMES[kind] + "_")]
    assert len(names) >= 10
    for name in names:
        c = pgd.case_inputs(Z, name)
        assert c["kind"] == kind
        _check_case(ctx, c, path, f"{name} {path}")


@pytest.mark.parametrize("kind", [9, 10])
def test_rational_quadratic_kinds(ctx, kind):
    """(130, 129), D = 3 against the dense helper; the fixture's own RQ cases, where it has any, against their 50 digits."""
    _check_case(ctx, make_case(kind, 130, 129, 3, seed=9200 + kind), "standalone", f"kind {kind}", golden=False)
    for name in RQ_NAMES:
        c = pgd.case_inputs(Z, name)
        if c["kind"] == kind:
            _check_case(ctx, c, "standalone", name)


@pytest.mark.parametrize("kind", [0, 1, 8, 10])
def test_a_column_does_not_depend_on_q(ctx, kind):
    """Column q of a Q = 3 call is the same bits inside Q = 17 (Qpad 16 -> 32) and Q = 70 (past one accumulator group of
    columns), at (130, 129), D = 3."""
    c = make_case(kind, 130, 129, 3, seed=9300 + kind)
    _single(ctx, c, "standalone")
    Y, mean = _columns(c, 70, 9350)
    out = {}
    for Q in (3, 17, 70):
        ctx.solve_targets(Y[:, :Q], mean[None, :Q])
        out[Q] = ctx.predict_targets_gradients()
        assert out[Q].shape == (129, 3, Q)
    assert _same_bits(out[3], out[17][:, :, :3]) and _same_bits(out[3], out[70][:, :, :3])
    assert _same_bits(out[17], out[70][:, :, :17])
    ref, tol = _dense(ctx, 0, c, Y, mean)
    _check(f"kind {kind} Q = 70", out[70], ref, 2.0 * tol)
    # other values in the other columns: column 1 keeps its bits
    Y2 = Y[:, :17].copy(order="F")
    Y2[:, 0] *= -3.0
    Y2[:, 2:] += 1.0
    ctx.solve_targets(Y2, mean[None, :17])
    assert _same_bits(ctx.predict_targets_gradients()[:, :, 1], out[3][:, :, 1])


def test_more_than_one_slab_of_training_rows(ctx):
    """n = 1500 (two slabs of training rows per test tile), n_t = 400, D = 8, IsoSE, against the dense helper."""
    n, nt, D = 1500, 400, 8
    X, y, Xt = dsm.regression_data(n, D, n_test=nt, seed=777)
    c = dict(X=np.asfortranarray(X), y=y, Xt=np.asfortranarray(Xt), mean=float(np.mean(y)), kind=0,
             loghyp=np.array([np.log(0.9), 0.0]), logNoise=float(np.log(0.1)))
    _single(ctx, c, "standalone")
    Y, mean = _columns(c, 3, 9400)
    ctx.solve_targets(Y, mean[None, :])
    dmu = ctx.predict_targets_gradients()
    ref, tol = _dense(ctx, 0, c, Y, mean)
    _check("n1500", dmu, ref, 2.0 * tol)
    assert _same_bits(dmu, ctx.predict_targets_gradients())
    print(f"predict_targets_gradients device seconds {ctx.predict_targets_gradients_seconds:.3g}")


def _table_targets(Q=3):
    T = TABLE
    Y, _ = _columns(dict(X=T["X"], y=T["y"], mean=0.0), Q, 9500)
    L = T["kid"].size
    mean = np.stack([np.mean(Y[T["obs_idx"][int(T["obs_ptr"][l]):int(T["obs_ptr"][l + 1])]], axis=0) for l in range(L)])
    mean[:, 0] = T["mean"]
    return Y, mean


def _table_reference(ctx, Y, mean):
    """(dmu, tolerance) over the entries of the 41-leaf table: the dense helper fed with download_factor of `ctx`."""
    T = TABLE
    rp, ri, op_, ob = T["route_ptr"], T["route_idx"], T["obs_ptr"], T["obs_idx"]
    E, D, Q = int(rp[-1]), T["X"].shape[1], Y.shape[1]
    ref, tol = np.zeros((E, D, Q)), np.ones((E, D, Q))
    for l in range(T["kid"].size):
        if rp[l + 1] == rp[l]:
            continue
        kid = int(T["kid"][l])
        hyp = T["hyp"][kid][:T["hyp_len"][kid]]
        o = ob[op_[l]:op_[l + 1]]
        c = dict(kind=int(T["kinds"][kid]), loghyp=hyp[:-1], logNoise=float(hyp[-1]), X=np.asfortranarray(T["X"][o]),
                 Xt=np.asfortranarray(T["Xt"][ri[rp[l]:rp[l + 1]]]))
        ref[int(rp[l]):int(rp[l + 1])], tol[int(rp[l]):int(rp[l + 1])] = _dense(ctx, l, c, Y[o], mean[l])
    return ref, tol


@pytest.mark.parametrize("lanes", [1, 2])
def test_leaf_table(ctx, lanes):
    """The 41-leaf table of gp_pred.npz (a COPY and a PREFIX leaf, a leaf without routed rows, four kernel ids): every leaf
    against the dense helper fed with download_factor of the same context, within twice the tolerance."""
    T = TABLE
    rp, ri = T["route_ptr"], T["route_idx"]
    assert np.any(T["op"] != 0) and np.any(np.diff(rp) == 0)
    Y, mean = _table_targets()
    ctx.set_option(hipabi.OPT_LANES, lanes)
    try:
        _table_setup(ctx)
        _, info, _ = ctx.fit()
        ctx.predict_leaves(T["Xt"], rp, ri)
        assert np.all(info == 0) and ctx.lanes() == lanes
        ctx.solve_targets(Y, mean)
        dmu = ctx.predict_targets_gradients()
        assert dmu.shape == (int(rp[-1]), T["X"].shape[1], 3)
        ref, tol = _table_reference(ctx, Y, mean)
        _check(f"table lanes={lanes}", dmu, ref, 2.0 * tol)
        assert _same_bits(dmu, ctx.predict_targets_gradients())
    finally:
        ctx.set_option(hipabi.OPT_LANES, 0)


def test_failed_leaf_gives_nan_rows_and_the_others_keep_their_bits(ctx):
    """Leaf 0: a rank-1 linear Gram of size 1e16 (not positive definite in float64, as tests/test_targets_gpu.py builds it); leaf
    1: an ordinary IsoSE leaf, whose entries are the bits of the same table with a leaf 0 that factorises."""
    n0, n1, nt = 140, 100, 9
    rng = np.random.default_rng(5)
    X = np.concatenate([np.linspace(1.0, 2.0, n0) * 1e8, rng.uniform(size=n1)]).reshape(-1, 1)
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(n1)])
    Y = np.stack([y, np.cos(X[:, 0]) + 3.0], axis=1)
    mean = np.array([[0.0, 0.0], [0.2, 3.5]])
    Xt = np.linspace(0.05, 0.95, nt).reshape(-1, 1)
    hyp1 = np.array([np.log(0.3), 0.0, np.log(0.1)])

    def run(fail):
        ctx.set_train(X, y)
        ctx.set_leaves([0, n0, n0 + n1], np.arange(n0 + n1), [0, 1], [0.0, 0.2])
        if fail:
            ctx.set_hyper(0, 2, [0.0, 0.0, -30.0])
        else:
            ctx.set_hyper(0, 0, hyp1)
        ctx.set_hyper(1, 0, hyp1)
        _, info, _ = ctx.fit()
        assert (info[0] != 0) == fail and info[1] == 0
        ctx.predict_leaves(Xt, [0, nt, 2 * nt], np.concatenate([np.arange(nt), np.arange(nt)]))
        ctx.solve_targets(Y, mean)
        return ctx.predict_targets_gradients()

    bad, good = run(True), run(False)
    assert np.all(np.isnan(bad[:nt])) and np.all(np.isfinite(bad[nt:])) and np.all(np.isfinite(good))
    assert _same_bits(bad[nt:], good[nt:])
    c = dict(kind=0, X=np.asfortranarray(X[n0:]), Xt=np.asfortranarray(Xt), loghyp=hyp1[:2], logNoise=hyp1[2])
    ref, tol = _dense(ctx, 1, c, Y[n0:], mean[1])
    _check("good leaf", bad[nt:], ref, 2.0 * tol)


def _code(fn):
    with pytest.raises(hipabi.DsmgpError) as e:
        fn()
    return e.value.code


def test_states_and_arguments():
    c = make_case(0, 40, 16, 2, seed=9600)
    X, Xt, n, nt = c["X"], c["Xt"], 40, 16
    Y, mean = _columns(c, 3, 9650)
    hyp = np.concatenate([c["loghyp"], [c["logNoise"]]])
    ctx = hipabi.Context(0)
    try:
        ctx.set_train(X, c["y"])
        ctx.set_leaves([0, n], np.arange(n), [0], [c["mean"]])
        ctx.set_hyper(0, 0, hyp)
        ctx.targets_Q = 3
        ctx.fit()
        ctx.predict_leaves(Xt, [0, nt], np.arange(nt))
        assert _code(ctx.predict_targets_gradients) == hipabi.E_STATE          # before solve_targets
        ctx.solve_targets(Y, mean[None, :])
        ctx.set_test(Xt[:8], [0, 8], np.arange(8))
        assert _code(ctx.predict_targets_gradients) == hipabi.E_STATE          # before predict_run
        ctx.set_test(Xt, [0, nt], np.arange(nt))
        ctx.predict_run()
        ref = ctx.predict_targets_gradients()
        buf = np.empty((nt, 2, 3), order="F")
        pb = buf.ctypes.data_as(C.POINTER(C.c_double))
        assert ctx.lib.dsmgp_predict_columns_gradients(ctx.h, pb, nt - 1, None) == hipabi.E_ARG      # ld < route_total
        assert ctx.lib.dsmgp_predict_columns_gradients(ctx.h, None, nt, None) == hipabi.E_ARG
        assert ctx.lib.dsmgp_predict_columns_gradients(ctx.h, pb, nt, None) == 0                     # seconds NULL
        assert _same_bits(buf, ref)
        wide = np.full((nt + 5, 2, 3), -7.0, order="F")                                                  # ld > route_total
        assert ctx.lib.dsmgp_predict_columns_gradients(ctx.h, wide.ctypes.data_as(C.POINTER(C.c_double)), nt + 5, None) == 0
        assert _same_bits(wide.reshape(nt + 5, 6, order="F")[:nt], ref.reshape(nt, 6, order="F")) and np.all(wide[nt:] == -7.0)
        ctx.fit()                                                               # a later fit: Z and the rows are stale
        assert _code(ctx.predict_targets_gradients) == hipabi.E_STATE
        ctx.predict_run()
        assert _code(ctx.predict_targets_gradients) == hipabi.E_STATE          # still no solve_targets on this fit
        ctx.solve_targets(Y, mean[None, :])
        assert _same_bits(ctx.predict_targets_gradients(), ref)                # the context stays usable
        hyp2 = hyp.copy()
        hyp2[0] += 0.1
        ctx.set_hyper(0, 0, hyp2)
        assert _code(ctx.predict_targets_gradients) == hipabi.E_STATE          # new hyper-parameters, no fit
        ctx.fit()
        ctx.solve_targets(Y, mean[None, :])
        ctx.predict_run()
        assert not _same_bits(ctx.predict_targets_gradients(), ref)
        ctx.set_test(Xt, [0, 0], np.zeros(0, dtype=np.int64))                  # no routed rows at all
        ctx.predict_run()
        assert ctx.predict_targets_gradients().shape == (0, 2, 3)              # success, nothing written
    finally:
        ctx.close()


def test_nothing_else_moves(ctx):
    """predict_fetch, predict_cov, predict_targets, targets_fetch, gradients, loo, predict_gradients and targets_gradients return
    the same bits before and after the call; so does gradients under a mask of set_gradient_leaves that leaves owners out, with
    the L^-T arena filled by the call itself."""
    T = TABLE
    L = T["kid"].size
    rp, ri = T["route_ptr"], T["route_idx"]
    Y, mean = _table_targets()
    stride = int(np.max(T["hyp_len"]))
    W = np.random.default_rng(3).uniform(-1.0, 2.0, size=(L, 3))
    leaf = int(np.argmax(np.diff(rp)))
    mask = np.zeros(L, dtype=np.int32)
    mask[[3, 7]] = 1

    def everything(call):
        _table_setup(ctx)
        ctx.fit()
        ctx.predict_leaves(T["Xt"], rp, ri)
        ctx.solve_targets(Y, mean)
        d = ctx.predict_targets_gradients() if call else None
        out = [*ctx.predict_fetch(), ctx.predict_cov(leaf, int(rp[leaf + 1] - rp[leaf])), ctx.predict_targets(),
               ctx.targets_fetch(0), ctx.targets_fetch(L - 1), ctx.gradients(stride), *ctx.loo(), *ctx.predict_gradients(),
               ctx.targets_gradients(stride, W)]
        if call:
            assert _same_bits(d, ctx.predict_targets_gradients())           # L^-T filled by the call, then read as it is
        # a fresh fit under the mask: the call inverts every owner over lists of its own
        _table_setup(ctx)
        ctx.set_gradient_leaves(mask)
        try:
            ctx.fit()
            ctx.predict_leaves(T["Xt"], rp, ri)
            ctx.solve_targets(Y, mean)
            if call:
                assert _same_bits(d, ctx.predict_targets_gradients())       # the mask does not apply
            masked = ctx.gradients(stride)
            assert np.all(masked[mask == 0] == 0.0)
            out += [masked, ctx.gradients(stride), *ctx.predict_fetch()]
        finally:
            ctx.set_gradient_leaves(None)
        return out

    base = everything(False)
    got = everything(True)
    assert len(base) == len(got)
    for k, (p, q) in enumerate(zip(base, got)):
        assert _same_bits(p, q), k
