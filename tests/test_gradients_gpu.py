"""GPU suite: the gradient pass (dsmgp_gradients) against 50-digit references, finite differences and the f64 oracle.

The pass is the blocked L^-T inversion, frob_kernel (tr K_y^-1), tile_graddot_kernel (the contraction, three epilogue
branches: ArdSE per dimension, coordinates staged through LDS for D <= GRADDOT_STAGE_D = 35, read from global memory
above), dots_kernel, ardlin_quad_kernel and the host assembly.  The cases reach every branch, the tile edges of the leaf
size (n = 1, 2, 127, 128, 129), the fused small-leaf steps, and every kernel kind in one partial-result buffer."""
import os

import numpy as np
import pytest
import scipy.linalg as sla

from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd.datagen import uniform, normal, regression_data
from oracle import gp as ogp
from dense_gp import DenseGP

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
STAGE_D = 35          # kernels.hpp GRADDOT_STAGE_D


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


def _single(ctx, X, y, mean, kind, hyp):
    """One leaf holding every row; hyp = the library hyper-vector including logNoise.  Returns the log-marginal."""
    n = X.shape[0]
    ctx.set_train(X, y)
    ctx.set_leaves([0, n], np.arange(n), [0], [mean])
    ctx.set_hyper(0, kind, hyp)
    mll, info, _ = ctx.fit()
    assert info[0] == 0
    return mll[0]


def _oracle(X, y, mean, kind, hyp):
    """f64 oracle of one leaf (DenseGP for ArdLinear)."""
    hyp = np.asarray(hyp, dtype=np.float64)
    if kind == 3:
        return DenseGP(3, hyp, X, y, mean)
    return ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, hyp[:-1]), hyp[-1], exact_dist=True).update_cholesky()


def _ardse_true_dl(go, dims):
    """0.5 tr((alpha alpha^T - K_y^-1) dK/dlog l_d) of an oracle ArdSE leaf: the DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT value."""
    Kinv = sla.cho_solve((go.L(), True), np.eye(go.N))
    P = np.outer(go.alpha, go.alpha) - Kinv
    ls = go.kernel.lengthscale() ** 2
    out = []
    for d in dims:
        q = go.P[:, :, d] / ls[d]
        out.append(0.5 * np.sum(P * go.kernel.variance() * np.exp(-0.5 * q) * q))
    return np.array(out)


# ------------------------------------------------------------------------------------- 1. the 50-digit fixture

def _grad_cases():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "gp_grad.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split("/")
        cases.setdefault(name, {})[field] = z[key]
    return cases


_CASES = _grad_cases()


def _tolerance(c, ref):
    """Per component: 64 cond_2(K_y) eps max(1, |g_mp|_inf), floored at 1e-13.  Weak-signal cases (sigma^2 / c = 1e-8) also
    allow the floor of the identity the host uses for tr(P K) = (y.alpha - c alpha.alpha) - (n - c tr K_y^-1): its two halves
    are each of size n + c tr K_y^-1 and cancel to a value ~ sigma^2 / c smaller, so it loses ~8 eps (n + c tr K_y^-1) absolutely
    (CPU-measured in NumPy against an 80-bit Cholesky, IsoSE D = 2: relative error 2e-12 at sigma^2/c = 1e-4, 1.9e-8 at 1e-8;
    a direct contraction stays at 1e-15).  That term enters IsoSE ds times sigma and IsoLinear dl times 1."""
    tol = np.full(ref.size, max(1e-13, 64.0 * float(c["cond"]) * EPS * max(1.0, float(np.max(np.abs(ref))))))
    if bool(c["weak"]):
        kind = int(c["kind"])
        floor = 8.0 * EPS * (float(c["n"]) + float(c["c_trKinv"]))
        if kind == 0:
            tol[1] += floor * np.exp(float(c["loghyp"][1]))
        elif kind == 2:
            tol[0] += floor
    return tol


@pytest.mark.parametrize("fused_gram", [0, 1])
@pytest.mark.parametrize("name", sorted(_CASES))
def test_gradients_against_50_digit_references(ctx, name, fused_gram):
    """tests/golden/gp_grad.npz (make_grad_golden.py): every component within its tolerance of the mpmath value, with the
    Gram values from the Gram launch and fused into the update tasks; ArdSE with the true length-scale gradient off
    (exact zeros) and on."""
    c = _CASES[name]
    kind = int(c["kind"])
    hyp = np.concatenate([c["loghyp"], [float(c["logNoise"])]])
    D = c["X"].shape[1]
    ctx.set_option(hipabi.OPT_FUSED_GRAM, fused_gram)
    try:
        variants = [(0, c["grad"])]
        if kind == 1:
            variants.append((1, np.concatenate([c["grad_true"], c["grad"][D:]])))
        for ard, ref in variants:
            ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, ard)
            try:
                mll = _single(ctx, c["X"], c["y"], float(c["mean"]), kind, hyp)
                g = ctx.gradients(hyp.size)[0]
            finally:
                ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
            assert abs(mll - float(c["mll"])) <= max(1e-13, 64.0 * float(c["cond"]) * EPS * max(1.0, abs(float(c["mll"]))))
            if kind == 1 and not ard:
                assert np.all(g[:D] == 0.0)
            tol = _tolerance(c, ref)
            err = np.abs(g - ref)
            print(f"\n{name} fused_gram={fused_gram} ard={ard}: max err {np.max(err):.3g}, worst err/tol {np.max(err / tol):.3g}")
            assert np.all(err <= tol), (name, ard, g, ref, tol)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_GRAM, 1)


# ------------------------------------------------------------------------------------- 2. finite differences, wide inputs

def _fd(ctx, X, y, mean, kind, hyp, j, e=1e-5):
    hp, hm = hyp.copy(), hyp.copy()
    hp[j] += e
    hm[j] -= e
    return (_single(ctx, X, y, mean, kind, hp) - _single(ctx, X, y, mean, kind, hm)) / (2 * e)


@pytest.mark.parametrize("D", [36, 48, 64])
@pytest.mark.parametrize("n", [700, 1111])
def test_isose_wide_input_gradients_against_finite_differences_and_the_oracle(ctx, D, n):
    """IsoSE above GRADDOT_STAGE_D: the contraction epilogue reads the coordinates from global memory.  n = 700 ends on a
    ragged row tile (60 rows), n = 1111 on one of <= 32 rows (87)."""
    X = uniform(7000 + D + n, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) + np.cos(2.0 * X[:, 1]) + 0.1 * normal(7100 + D + n, 0, n)
    mean = float(np.mean(y))
    hyp = np.array([np.log(0.3 * np.sqrt(D)), 0.1, np.log(0.2)])
    _single(ctx, X, y, mean, 0, hyp)
    g = ctx.gradients(3)[0]
    assert ctx.work_gradients()[2] > 0            # contraction tasks exist: D > 35 runs the global-memory branch
    sigma = np.exp(hyp[1])
    for j, scale in ((0, sigma), (1, sigma), (2, 1.0)):
        fd = _fd(ctx, X, y, mean, 0, hyp, j)
        assert abs(g[j] / scale - fd) <= 2e-6 * max(1.0, abs(fd)), (j, g[j] / scale, fd)
    go = _oracle(X, y, mean, 0, hyp).grad()
    assert np.max(np.abs(g - go)) <= 1e-9 * max(1.0, float(np.max(np.abs(go)))), (g, go)


def test_isolinear_wide_input_gradients_against_finite_differences_and_the_oracle(ctx):
    n, D = 700, 48
    X = uniform(7200, 0, n * D).reshape((n, D), order="F")
    y = X[:, :4].sum(axis=1) - 2.0 + 0.1 * normal(7201, 0, n)
    mean = float(np.mean(y))
    hyp = np.array([np.log(2.0 * np.sqrt(D)), 0.0, np.log(0.2)])
    _single(ctx, X, y, mean, 2, hyp)
    g = ctx.gradients(3)[0]
    assert g[1] == 0.0
    for j in (0, 2):
        fd = _fd(ctx, X, y, mean, 2, hyp, j)
        assert abs(g[j] - fd) <= 2e-6 * max(1.0, abs(fd)), (j, g[j], fd)
    go = _oracle(X, y, mean, 2, hyp).grad()
    assert np.max(np.abs(g - go)) <= 1e-9 * max(1.0, float(np.max(np.abs(go)))), (g, go)


def test_ardse_true_lengthscale_gradient_at_the_staging_limit(ctx):
    """ArdSE, DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT on, D = 35: coordinates and alpha fill the LDS ring exactly
    ((35 + 1) x 256 doubles); 4 sampled dimensions against finite differences and the oracle's direct contraction."""
    n, D = 700, STAGE_D
    X = uniform(7300, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) + np.cos(2.0 * X[:, 34]) + 0.1 * normal(7301, 0, n)
    mean = float(np.mean(y))
    hyp = np.array(list(np.log(np.linspace(0.3, 1.2, D))) + [-0.5 * np.log(D), np.log(0.2)])
    dims = [0, 11, 22, 34]
    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
    try:
        _single(ctx, X, y, mean, 1, hyp)
        g = ctx.gradients(D + 2)[0]
        for d in dims:
            fd = _fd(ctx, X, y, mean, 1, hyp, d)
            assert abs(g[d] - fd) <= 2e-6 * max(1.0, abs(fd)), (d, g[d], fd)
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    go = _oracle(X, y, mean, 1, hyp)
    ref = np.concatenate([_ardse_true_dl(go, dims), go.grad()[D:]])
    got = np.concatenate([g[dims], g[D:]])
    assert np.max(np.abs(got - ref)) <= 1e-9 * max(1.0, float(np.max(np.abs(ref)))), (got, ref)


# ------------------------------------------------------------------------------------- 3. the ArdSE refusal

def test_ardse_option_refusal_above_the_staging_limit_leaves_a_usable_context(ctx):
    """D = 36 with the true ArdSE gradient: DSMGP_E_ARG naming the limit (a host check: the task lists are uploaded, no
    kernel runs).  The same context then gives, bit for bit, what a fresh context gives: ArdSE with the option off, and
    IsoSE on kernel id 0."""
    n, D = 300, STAGE_D + 1
    X = uniform(7400, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) + 0.1 * normal(7401, 0, n)
    mean = float(np.mean(y))
    ard = np.array(list(np.log(np.linspace(0.5, 1.5, D))) + [-0.5 * np.log(D), np.log(0.2)])
    iso = np.array([np.log(0.3 * np.sqrt(D)), 0.0, np.log(0.2)])
    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
    try:
        _single(ctx, X, y, mean, 1, ard)
        with pytest.raises(hipabi.DsmgpError) as ei:
            ctx.gradients(D + 2)
        assert ei.value.code == hipabi.E_ARG and f"D <= {STAGE_D}" in str(ei.value)
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    g_ard = ctx.gradients(D + 2)          # same fit, option off
    ctx.set_hyper(0, 0, iso)
    ctx.fit()
    g_iso = ctx.gradients(3)
    fresh = hipabi.Context(0)
    try:
        _single(fresh, X, y, mean, 1, ard)
        f_ard = fresh.gradients(D + 2)
        fresh.set_hyper(0, 0, iso)
        fresh.fit()
        f_iso = fresh.gradients(3)
    finally:
        fresh.close()
    assert np.all(g_ard[0, :D] == 0.0) and np.array_equal(g_ard, f_ard)
    assert np.array_equal(g_iso, f_iso)
    go = _oracle(X, y, mean, 0, iso).grad()
    assert np.max(np.abs(g_iso[0] - go)) <= 1e-9 * max(1.0, float(np.max(np.abs(go))))


# ------------------------------------------------------------------------------------- 4. fused against classic steps

_HYP = {0: [np.log(0.3), 0.0, np.log(0.2)],
        1: [np.log(0.3), np.log(0.4), np.log(0.5), -0.5 * np.log(3.0), np.log(0.2)],
        2: [np.log(1.5), 0.0, np.log(0.2)],
        3: [np.log(1.2), np.log(1.5), np.log(1.8), 0.0, np.log(0.2)]}


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_fused_steps_give_the_gradients_of_the_classic_steps(ctx, kind):
    """A table of 600 leaves of 130..520 rows has more diagonal blocks per step than the chip has CUs: its block steps run
    fused (diag_fused_reg_kernel + tile_fused8_kernel) and the gradient pass takes its Dinv_k from ensure_dinv.  With
    DSMGP_OPT_FUSED_STEPS = 0 the same table runs classic steps.  Last row tiles of every class (<= 32, <= 64, <= 96, whole),
    a COPY and a PREFIX leaf; ArdSE with the true length-scale gradient.  Per leaf 1e-11 relative; one leaf of each row class
    against the oracle at 1e-9."""
    N, D, L = 40_000, 3, 600
    X, y, _ = regression_data(N, D, n_test=1, seed=7500 + kind)
    rng = np.random.default_rng(75 + kind)
    sizes = rng.integers(130, 521, size=L)
    sizes[:8] = [130, 160, 192, 224, 256, 300, 352, 384]        # last row tile: 2, 32, 64, 96, 128, 44, 96, 128 rows
    obs = [np.sort(rng.choice(N, size=int(n), replace=False)) for n in sizes]
    obs[10] = obs[3].copy()                                       # COPY of leaf 3
    tail = np.arange(obs[5][-1] + 1, min(N, obs[5][-1] + 1 + 230))
    obs[11] = np.concatenate([obs[5], tail])                      # PREFIX: leaf 5 is its leading part
    op = np.zeros(L, dtype=np.int32)
    src = np.full(L, -1, dtype=np.int32)
    plen = np.zeros(L, dtype=np.int64)
    op[10], src[10] = 1, 3
    if tail.size:
        op[11], src[11], plen[11] = 2, 5, obs[5].size
    means = [float(np.mean(y[o])) for o in obs]
    means[10] = means[3]
    hyp = np.array(_HYP[kind])
    stride = hyp.size

    def run(fused):
        ctx.set_option(hipabi.OPT_FUSED_STEPS, fused)
        ctx.set_train(X, y)
        ctx.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in obs])]), np.concatenate(obs), np.zeros(L, dtype=np.int32), means)
        ctx.set_sharing(op, src, plen)
        ctx.set_hyper(0, kind, hyp)
        ctx.set_profile(2)
        _, info, _ = ctx.fit()
        assert np.all(info == 0)
        t = ctx.timings()
        return ctx.gradients(stride), t

    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
    try:
        ga, ta = run(1)
        gb, tb = run(0)
    finally:
        ctx.set_option(hipabi.OPT_FUSED_STEPS, 1)
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
        ctx.set_profile(0)
    assert ta["gram"] < 0.5 * tb["gram"]             # the fused run had no Gram launch: its steps ran fused
    scale = np.max(np.abs(gb), axis=1)
    assert np.all(scale > 0)
    rel = np.max(np.abs(ga - gb), axis=1) / scale
    assert np.all(rel <= 1e-11), (int(np.argmax(rel)), float(np.max(rel)))
    assert np.allclose(ga[10], ga[3], rtol=1e-12, atol=0)   # the COPY leaf with its source's mean: its source's gradients
    for j in (1, 2, 3, 4, 10, 11):                   # row classes <= 32, <= 64, <= 96, whole; the COPY and the PREFIX leaf
        go = _oracle(X[obs[j]], y[obs[j]], means[j], kind, hyp)
        ref = go.grad()
        if kind == 1:
            ref[:D] = _ardse_true_dl(go, range(D))
        assert np.max(np.abs(ga[j] - ref)) <= 1e-9 * max(1.0, float(np.max(np.abs(ref)))), (j, ga[j], ref)


# ------------------------------------------------------------------------------------- 5. every kind in one context

def test_every_kernel_kind_in_one_context_equals_each_leaf_alone(ctx):
    """Kernel ids 0..3 = IsoSE, ArdSE (true length-scale gradient: gstride = 2 + D), IsoLinear, ArdLinear in one leaf
    table, leaves of n = 1, 2, 127, 128, 129, 300 for each, and COPY leaves: with their source's mean (they take the
    source's contraction / ArdLinear sums) and with a mean of their own (they do not).  The partial-result buffer
    frob | graddot x gstride | dots | ardlin holds every part at once.  Each row equals the same leaf fitted alone to
    1e-12 relative (not bitwise: task dealing reorders the sums); with a gradient mask the rows left out are exactly zero."""
    N, D = 3000, 3
    X, y, _ = regression_data(N, D, n_test=1, seed=7600)
    rng = np.random.default_rng(76)
    obs, kid, means = [], [], []
    for k in range(4):
        for n in (1, 2, 127, 128, 129, 300):
            o = np.sort(rng.choice(N, size=n, replace=False))
            obs.append(o)
            kid.append(k)
            means.append(float(np.mean(y[o])) if n > 1 else 0.0)
    L0 = len(obs)
    op = [0] * L0
    src = [-1] * L0
    # COPY leaves: IsoSE n = 300 and ArdLinear n = 129 with the source's mean; ArdSE n = 128 and IsoLinear n = 127 with their own
    for s, own in ((5, False), (22, False), (9, True), (14, True)):
        obs.append(obs[s].copy())
        kid.append(kid[s])
        means.append(means[s] + (0.3 if own else 0.0))
        op.append(1)
        src.append(s)
    L = len(obs)
    stride = D + 2
    ptr = np.concatenate([[0], np.cumsum([o.size for o in obs])])

    def setup(c, leaves):
        c.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
        c.set_train(X, y)
        sel = [obs[i] for i in leaves]
        c.set_leaves(np.concatenate([[0], np.cumsum([o.size for o in sel])]), np.concatenate(sel),
                     [kid[i] for i in leaves], [means[i] for i in leaves])
        for k in range(4):
            c.set_hyper(k, k, _HYP[k])

    mixed = hipabi.Context(0)
    try:
        setup(mixed, range(L))
        assert ptr[-1] == sum(o.size for o in obs)
        mixed.set_sharing(op, src, np.zeros(L, dtype=np.int64))
        _, info, _ = mixed.fit()
        assert np.all(info == 0)
        full = mixed.gradients(stride)
        active = np.zeros(L, dtype=bool)
        active[[0, 3, 7, 14, 19, 23, 25, 26]] = True       # 25: COPY of 22 (inactive) with 22's mean; 26: own-mean COPY of 9
        mixed.set_gradient_leaves(active)
        masked = mixed.gradients(stride)
    finally:
        mixed.close()
    assert np.all(masked[~active] == 0.0)
    try:
        alone = np.zeros((L, stride))
        for i in range(L):
            setup(ctx, [i])
            _, info, _ = ctx.fit()
            assert info[0] == 0
            alone[i] = ctx.gradients(stride)[0]
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    scale = np.max(np.abs(alone), axis=1)
    assert np.all(scale > 0)
    for g in (full, masked):
        rows = np.arange(L) if g is full else np.flatnonzero(active)
        rel = np.max(np.abs(g[rows] - alone[rows]), axis=1) / scale[rows]
        assert np.all(rel <= 1e-12), (int(rows[np.argmax(rel)]), float(np.max(rel)))
    for i in range(L):                                 # slots past the hyper-vector stay zero (IsoSE, IsoLinear: 3 used)
        assert np.all(full[i, len(_HYP[kid[i]]):] == 0.0)
    assert np.allclose(full[24], full[5], rtol=1e-12, atol=0) and np.allclose(full[25], full[22], rtol=1e-12, atol=0)
    assert np.max(np.abs(full[26] - full[9])) > 1e-6 and np.max(np.abs(full[27] - full[14])) > 1e-6
