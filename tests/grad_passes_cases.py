"""The cases whose raw float64 outputs tests/golden/grad_passes_parent.npz records from the four hyper-parameter gradient entry
points (dsmgp_gradients, dsmgp_loo_gradients, dsmgp_mll_columns_gradients, dsmgp_loo_columns_gradients): the smallest shapes at
which the order of the contraction task list, its dealing to the XCDs or the host reduction can go wrong (TB = 128, super-tiles
of 4 x 4 tiles).  Shared by the recorder tests/golden/make_grad_passes_parent.py and by tests/test_grad_passes_bits_gpu.py,
which asserts the recorded bits.  Inputs come from datagen's counter streams: no library generator whose stream could change.

    single/<kind>/n<n>      one leaf, D = 3: every kind at n = 300; n = 1, 130, 600 (5 blocks: a super-tile boundary in both tile
                            indices) for IsoSE, ArdLinear, ArdMatern52 and ArdRQ
    single/ArdSE-true/n300  ArdSE with OPT_ARD_LENGTHSCALE_GRADIENT on
    mixed                   nine leaves on the rows of tests/sharing_tables.py: IsoSE 130, ArdSE 300, ArdLinear 600, ArdSEProduct
                            300, IsoMatern32 257, ArdRQ 300; a COPY leaf of the IsoSE leaf with its mean and one with a mean of its
                            own; a PREFIX leaf (300 -> 385) of the ArdSE leaf.  All four kernel ranges are non-empty, the dealing
                            mixes leaves, and the gradient mask, the shared sums of a COPY leaf and the call-to-call protocol of
                            the L^-T arena are exercised
    wide                    n = 130, D = 40, ArdSEProduct (chunked staging): gradients and targets_gradients only

Every fit must give info = 0 (asserted here).  Test infrastructure only."""
import numpy as np

import sharing_tables as st
from deepstructuredmixtures_amd import hipabi

KIND_NAMES = ("IsoSE", "ArdSE", "IsoLinear", "ArdLinear", "ArdSEProduct", "IsoMatern32", "IsoMatern52", "ArdMatern32",
              "ArdMatern52", "IsoRQ", "ArdRQ")
# the library hyper-vectors at D = 3 (with logNoise), as tests/test_loo_columns_gpu.py has them (_HYP): well conditioned
HYP = [
    [np.log(0.4), 0.1, np.log(0.2)],
    list(np.log([0.4, 0.6, 0.9])) + [-0.3, np.log(0.2)],
    [np.log(1.0), 0.0, np.log(0.2)],
    list(np.log([0.8, 1.2, 1.6])) + [0.0, np.log(0.2)],
    list(np.log([0.5, 0.7, 0.9])) + [0.0, np.log(0.2)],
    [np.log(0.5), 0.0, np.log(0.2)],
    [np.log(0.7), 0.2, np.log(0.2)],
    list(np.log([0.5, 0.7, 0.9])) + [0.1, np.log(0.2)],
    list(np.log([0.5, 0.8, 0.6])) + [-0.1, np.log(0.2)],
    [np.log(0.5), np.log(2.0), 0.0, np.log(0.2)],
    list(np.log([0.5, 0.7, 0.9])) + [np.log(0.3), -0.1, np.log(0.2)],
]
SIZES = (1, 130, 300, 600)
ALL_SIZES_KINDS = (0, 3, 8, 10)


def columns(stream, X, Q):
    """Q target columns over the rows of X: smooth in the first input, different scales and offsets, 0.1 noise."""
    j = np.arange(Q)
    z = st.normal(stream, 0, X.shape[0] * Q).reshape((X.shape[0], Q), order="F")
    return np.sin((1.0 + j)[None, :] * X[:, :1]) * (1.0 + 0.5 * j)[None, :] + 3.0 * (j % 3)[None, :] + 0.1 * z


def _work(ctx):
    return np.array(ctx.work_gradients(), dtype=np.float64)


def _single(ctx, kind, n, D, hyp, true_ard=False, loo=True):
    X = np.asfortranarray(st.uniform(9100 + 16 * kind + (n % 16), 0, n * D).reshape((n, D), order="F"))
    Y = columns(9500 + kind, X, 3)
    mean = np.mean(Y, axis=0) + 0.05
    hyp = np.asarray(hyp, dtype=np.float64)
    out = {}
    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1 if true_ard else 0)
    try:
        ctx.set_train(X, Y[:, 0])
        ctx.set_leaves([0, n], np.arange(n), [0], [float(mean[0])])
        ctx.set_sharing(None, None, None)
        ctx.set_hyper(0, kind, hyp)
        _, info, _ = ctx.fit()
        assert info[0] == 0, (kind, n, info)
        out["gradients"] = ctx.gradients(hyp.size)
        out["work"] = _work(ctx)
        if loo:
            out["loo_gradients"], out["loo_lpd"] = ctx.loo_gradients(hyp.size)
        ctx.solve_targets(Y, mean[None, :])
        out["targets_gradients"] = ctx.targets_gradients(hyp.size)
        out["targets_gradients_w"] = ctx.targets_gradients(hyp.size, np.array([[0.5, -0.25, 1.75]]))
        if loo:
            out["loo_targets_gradients"], out["loo_targets_lpd"] = ctx.loo_targets_gradients(hyp.size)
            out["loo_targets_gradients_w"], _ = ctx.loo_targets_gradients(hyp.size, np.array([[0.5, 0.0, 1.75]]))
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    return out


# leaf -> (set of tests/sharing_tables.py, kind); then the COPY leaves of leaf 0 and the PREFIX leaf of leaf 1
MIXED_LEAVES = (("g129_130/leaf", 0), ("g300_385/src", 1), ("g256_257/600", 3), ("g127_300/leaf", 4), ("g256_257/leaf", 5),
                ("g128_129/300", 10))
MIXED_MASK_OFF = (0, 4)      # leaf 0 owns the factor of the COPY leaves 6 and 7 (6 takes its contraction sums too)


def _mixed(ctx):
    dat = st.data(3)
    sets = [dat.sets[k] for k, _ in MIXED_LEAVES]
    obs = [s["obs"] for s in sets] + [sets[0]["obs"], sets[0]["obs"], dat.sets["g300_385/leaf"]["obs"]]
    assert [o.size for o in obs] == [130, 300, 600, 300, 257, 300, 130, 130, 385]
    kid = [0, 1, 2, 3, 4, 5, 0, 0, 1]
    L = len(obs)
    op = np.array([0] * 6 + [st.COPY, st.COPY, st.PREFIX], dtype=np.int32)
    src = np.array([-1] * 6 + [0, 0, 1], dtype=np.int32)
    plen = np.array([0] * 8 + [300], dtype=np.int64)
    stride = 6
    ptr = np.concatenate([[0], np.cumsum([o.size for o in obs])])

    def means(Y):
        m = np.stack([np.mean(Y[o], axis=0) for o in obs])
        m[7] += st.OWN_MEAN_SHIFT                    # (row 6 is row 0's: the same rows)
        return m

    mean0 = means(dat.y[:, None])[:, 0]
    ctx.set_train(dat.X, dat.y)
    ctx.set_leaves(ptr, np.concatenate(obs), kid, mean0)
    for k, (_, kind) in enumerate(MIXED_LEAVES):
        ctx.set_hyper(k, kind, HYP[kind])
    ctx.set_sharing(op, src, plen)
    out = {}

    def fit():
        _, info, _ = ctx.fit()
        assert np.all(info == 0), info

    fit()
    out["gradients"] = ctx.gradients(stride)
    out["work"] = _work(ctx)
    mask = np.ones(L, dtype=np.int32)
    mask[list(MIXED_MASK_OFF)] = 0
    ctx.set_gradient_leaves(mask)
    try:
        out["gradients_mask"] = ctx.gradients(stride)
        out["loo_gradients_under_mask"], out["loo_lpd_under_mask"] = ctx.loo_gradients(stride)
        out["gradients_mask_after_loo"] = ctx.gradients(stride)
    finally:
        ctx.set_gradient_leaves(None)
    out["gradients_again"] = ctx.gradients(stride)
    out["loo_gradients"], out["loo_lpd"] = ctx.loo_gradients(stride)
    for Q in (3, 17):
        Y = np.concatenate([dat.y[:, None], columns(9700 + Q, dat.X, Q - 1)], axis=1)
        m = means(Y)
        m[:, 0] = mean0
        W = 2.0 * st.uniform(9800 + Q, 0, L * Q).reshape((L, Q), order="F")
        W[3] = 0.0                                   # a leaf without weight
        W[5, 1] = 0.0
        Wneg = W.copy()
        Wneg[2, Q - 1] = -0.75                       # any sign for the marginal likelihood
        ctx.solve_targets(Y, m)
        out[f"q{Q}/targets_gradients"] = ctx.targets_gradients(stride)
        out[f"q{Q}/targets_gradients_w"] = ctx.targets_gradients(stride, Wneg)
        out[f"q{Q}/loo_targets_gradients"], out[f"q{Q}/loo_targets_lpd"] = ctx.loo_targets_gradients(stride)
        out[f"q{Q}/loo_targets_gradients_w"], _ = ctx.loo_targets_gradients(stride, W)
        out[f"q{Q}/gradients_after"] = ctx.gradients(stride)
    # the true ArdSE length-scale gradient: the ArdSE leaves join the first kernel range of the two marginal-likelihood passes
    ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 1)
    try:
        fit()
        out["true_ard/gradients"] = ctx.gradients(stride)
        out["true_ard/work"] = _work(ctx)
        Y = np.concatenate([dat.y[:, None], columns(9703, dat.X, 2)], axis=1)
        m = means(Y)
        m[:, 0] = mean0
        ctx.solve_targets(Y, m)
        out["true_ard/targets_gradients"] = ctx.targets_gradients(stride)
    finally:
        ctx.set_option(hipabi.OPT_ARD_LENGTHSCALE_GRADIENT, 0)
    return out


def _wide(ctx):
    D = 40
    hyp = list(np.log(np.sqrt(D) * np.linspace(0.3, 0.6, D))) + [0.0, np.log(0.2)]
    return _single(ctx, 4, 130, D, hyp, loo=False)


def _make_cases():
    cases = {}
    for kind, name in enumerate(KIND_NAMES):
        for n in (SIZES if kind in ALL_SIZES_KINDS else (300,)):
            cases[f"single/{name}/n{n}"] = (lambda ctx, kind=kind, n=n: _single(ctx, kind, n, 3, HYP[kind]))
    cases["single/ArdSE-true/n300"] = lambda ctx: _single(ctx, 1, 300, 3, HYP[1], true_ard=True)
    cases["mixed"] = _mixed
    cases["wide"] = _wide
    return cases


CASES = _make_cases()      # name -> f(ctx) -> {array name: float64 array}


def run(name):
    """The arrays of one case, from a context of its own."""
    ctx = hipabi.Context(0)
    try:
        return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in CASES[name](ctx).items()}
    finally:
        ctx.close()
