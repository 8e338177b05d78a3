"""Leaf tables past one and two chunks of leaves, and a reference that shares nothing with the library.

Every launch with one grid row per leaf is cut into runs of 32,768 leaves (csrc/leaf_chunks.hpp).  A wrong first leaf of a run
gives leaf l the rows, test rows or target columns of leaf l - 32768; a grid row count that wraps at 16 bits does the same with
65,536.  The two tables here make either visible at the smallest shapes at which it exists.  Test infrastructure only.

    table("A")   L = 33,000: one chunk edge, with sharing across it and a failed leaf past it
    table("B")   L = 65,600: crosses 32,768, 65,535 and 65,536; the third chunk holds 64 leaves

Both from datagen's counter streams, D = 2:
    ordinary leaves   leaf l has 1 + l % 3 rows; all row sets are disjoint; obs_idx is a fixed permutation of the training rows
                      (sorted inside a leaf: the library wants ascending lists), so leaves l and l - 32768 share no row
    kernel ids        kid = l % 3: 0 IsoSE (kind 0), 1 ArdSEProduct (kind 4), 2 ArdLinear (kind 3), two distinct length-scales
                      for the ARD ids; noise 0.04 on unit-scale kernels: cond_2 of every 3 x 3 K_y is below 10^3 (asserted)
    means             mean of the leaf's y plus 0.01 (l % 7)
    larger leaves     index 0: 130 rows; 32,767: 130 rows; 32,768: 300 rows (npad = 384: the grid's first dimension is 2, and
                      classic steps run beside the fused step-0 tasks); L - 1: 130 rows
    sharing (A)       leaf 32,770 is a COPY of leaf 5 (its 3 rows, its kernel id 2) with another mean; leaf 32,771 is a PREFIX
                      leaf of leaf 32,767: the library's PREFIX takes the WHOLE source list, so it has the source's 130 rows,
                      of which the one complete 128-row block is copied (kb = 1), and 20 rows of its own after them (150 rows)
    failed leaf (A)   leaf 32,790 alone has kernel id 3: IsoLinear on 140 inputs of size 1e8 with logNoise = -30 (the rank-one
                      construction of tests/test_loo_gpu.py / test_kfold_gpu.py): info != 0 and NaN outputs
    test rows         6 each for about 400 leaves -- every leaf within 2 of 0, 32,767, 32,768, 65,535, 65,536 and L - 1, the
                      special leaves and the failed leaf's neighbours, 300 leaves drawn over the table and 50 over its last
                      chunk; each row lies within 0.1 of one of its leaf's training inputs, so another leaf's test rows give
                      another prediction; all other leaves have nt = 0
    targets           Q = 3 columns of the form of tests/grad_passes_cases.py::columns, the last one offset by 1000; the mean of
                      leaf l and column q is the leaf's mean of the column plus 0.01 (l % 7)
    folds             K = 2, label = training row % 2

`reference` evaluates every leaf of up to 3 rows in np.longdouble (eps 1.08e-19, asserted below): the three kernel functions
written out, an unrolled 3 x 3 Cholesky and substitutions on arrays over the leaf axis (a leaf of fewer rows is padded with an
identity block, which changes none of its results), no LAPACK call and nothing from oracle/, the dense helpers or the library.
`wrap` arguments evaluate it as a library would that took the rows, test rows or target rows of another leaf index (the start of
the list moves; the row count, kernel id and mean stay leaf l's: that is what a wrong leaf0 in a gather kernel does).

`tolerances` restates the project's tolerance rules over the leaf axis (tests/test_many_leaves_host.py checks them against the
functions they restate, leaf by leaf); `large_leaf` is the float64 dense reference of the 130-, 150- and 300-row leaves."""
import functools
import importlib.util
import os

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_many_leaves_datagen", os.path.join(_ROOT, "deepstructuredmixtures_amd", "datagen.py"))
_datagen = importlib.util.module_from_spec(_spec)      # the generator alone: importing the package would load the product
_spec.loader.exec_module(_datagen)
uniform, normal = _datagen.uniform, _datagen.normal

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not the 80-bit extended type here"
EPS = np.finfo(np.float64).eps
RTOL, ATOL = 1e-8, 1e-11                 # tests/pred_tolerance.py
JITTER = 1e-8
LOG2PI_LD = np.log(2 * np.arccos(LD(-1)))

CHUNK = 32768
FULL, COPY, PREFIX = 0, 1, 2
D, Q, NT, KFOLDS, STRIDE = 2, 3, 6, 2, 4
KINDS = (0, 4, 3, 2)                     # kernel id -> kind
HYP = ([np.log(0.4), 0.1, np.log(0.2)],
       [np.log(0.5), np.log(0.7), 0.0, np.log(0.2)],
       [np.log(0.8), np.log(1.2), 0.0, np.log(0.2)],
       [0.0, 0.0, -30.0])
COPY_SRC, COPY_LEAF, PREFIX_SRC, PREFIX_LEAF, FAILED = 5, CHUNK + 2, CHUNK - 1, CHUNK + 3, CHUNK + 22
SIZES = {"A": 33000, "B": 65600}
EDGES = (0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK)


class Table:
    pass


def columns(stream, X, nq):
    """tests/grad_passes_cases.py::columns: smooth in the first input, different scales and offsets, 0.1 noise."""
    j = np.arange(nq)
    z = normal(stream, 0, X.shape[0] * nq).reshape((X.shape[0], nq), order="F")
    return np.sin((1.0 + j)[None, :] * X[:, :1]) * (1.0 + 0.5 * j)[None, :] + 3.0 * (j % 3)[None, :] + 0.1 * z


@functools.lru_cache(maxsize=None)
def table(name):
    L, full = SIZES[name], name == "A"
    t = Table()
    t.name, t.L = name, L
    ls = np.arange(L)
    n = 1 + ls % 3
    kid = (ls % 3).astype(np.int32)
    t.big = {0: 130, CHUNK - 1: 130, CHUNK: 300, L - 1: 130}
    for l, v in t.big.items():
        n[l] = v
    own = n.copy()                           # rows drawn from the permutation
    tail = 0
    if full:
        n[FAILED] = own[FAILED] = 140
        kid[FAILED] = 3
        kid[COPY_LEAF], n[COPY_LEAF], own[COPY_LEAF] = kid[COPY_SRC], n[COPY_SRC], 0
        kid[PREFIX_LEAF], own[PREFIX_LEAF], tail = kid[PREFIX_SRC], 0, 20
        n[PREFIX_LEAF] = n[PREFIX_SRC] + tail
    n_perm = int(own.sum())
    N = n_perm + tail                        # the PREFIX leaf's own rows are the last ones: its list ascends
    perm = np.argsort(uniform(7101, 0, n_perm), kind="stable")
    leaf_of = np.repeat(ls, own)
    drawn = perm[np.lexsort((perm, leaf_of))]           # leaf by leaf, ascending inside a leaf
    optr = np.concatenate([[0], np.cumsum(own)])
    if full:
        c0 = int(optr[COPY_LEAF])                         # (= optr[PREFIX_LEAF]: neither draws)
        obs_idx = np.concatenate([drawn[:c0], drawn[optr[COPY_SRC]:optr[COPY_SRC + 1]],
                                  drawn[optr[PREFIX_SRC]:optr[PREFIX_SRC + 1]], np.arange(n_perm, N), drawn[c0:]])
    else:
        obs_idx = drawn
    t.n, t.kid, t.N = n, kid, N
    t.obs_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    t.obs_idx = obs_idx.astype(np.int64)
    assert t.obs_idx.size == t.obs_ptr[-1]
    X = uniform(7102, 0, N * D).reshape((N, D), order="F")
    y = np.sin(3.0 * X[:, 0]) + np.cos(2.0 * X[:, 1]) + 0.1 * normal(7103, 0, N)
    if full:
        rows = t.obs_idx[t.obs_ptr[FAILED]:t.obs_ptr[FAILED + 1]]
        X[rows, 0], X[rows, 1], y[rows] = np.linspace(1.0, 2.0, rows.size) * 1e8, 0.0, 0.0
    t.X, t.y = np.asfortranarray(X), y
    Y = columns(7104, X, Q)
    Y[:, Q - 1] += 1000.0
    t.Y = np.asfortranarray(Y)
    shift = 0.01 * (ls % 7)
    t.mean = np.add.reduceat(y[t.obs_idx], t.obs_ptr[:-1]) / n + shift
    t.Ymean = np.asfortranarray(np.add.reduceat(Y[t.obs_idx], t.obs_ptr[:-1], axis=0) / n[:, None] + shift[:, None])
    t.fold = (np.arange(N) % KFOLDS).astype(np.int32)
    # sharing
    t.op, t.src, t.plen = np.zeros(L, dtype=np.int32), np.full(L, -1, dtype=np.int32), np.zeros(L, dtype=np.int64)
    t.special = {}
    if full:
        t.op[COPY_LEAF], t.src[COPY_LEAF] = COPY, COPY_SRC
        t.op[PREFIX_LEAF], t.src[PREFIX_LEAF], t.plen[PREFIX_LEAF] = PREFIX, PREFIX_SRC, n[PREFIX_SRC]
        t.special = {"copy": COPY_LEAF, "copy_src": COPY_SRC, "prefix": PREFIX_LEAF, "prefix_src": PREFIX_SRC, "failed": FAILED}
    t.failed = FAILED if full else None
    t.small = np.flatnonzero(n <= 3)
    t.large = [int(l) for l in np.flatnonzero(n > 3) if l != t.failed]
    # routed leaves
    near = {e + d for e in EDGES + (L - 1,) for d in range(-2, 3)}
    last0 = (L - 1) // CHUNK * CHUNK
    drawn_l = set((uniform(7105, 0, 300) * L).astype(np.int64)) | set(last0 + (uniform(7106, 0, 50) * (L - last0)).astype(np.int64))
    extra = set(t.special.values()) | ({FAILED - 1, FAILED + 1} if full else set())
    t.routed = np.array(sorted(l for l in near | drawn_l | extra if 0 <= l < L), dtype=np.int64)
    t.edge_leaves = np.array(sorted(l for l in near | extra if 0 <= l < L), dtype=np.int64)
    nt = np.zeros(L, dtype=np.int64)
    nt[t.routed] = NT
    t.nt = nt
    t.route_ptr = np.concatenate([[0], np.cumsum(nt)]).astype(np.int64)
    n_t = int(t.route_ptr[-1])
    permt = np.argsort(uniform(7107, 0, n_t), kind="stable").reshape(-1, NT)
    permt.sort(axis=1)
    t.route_idx = permt.reshape(-1).astype(np.int64)
    Xt = np.empty((n_t, D))
    off = 0.2 * (uniform(7108, 0, n_t * D).reshape((n_t, D), order="F") - 0.5)
    for j in range(NT):                                 # test row j of a leaf: near its training row j % n
        e = t.route_ptr[t.routed] + j
        Xt[t.route_idx[e]] = X[t.obs_idx[t.obs_ptr[t.routed] + j % n[t.routed]]] + off[t.route_idx[e]]
    t.Xt, t.n_t = np.asfortranarray(Xt), n_t
    return t


def plan_bytes(t):
    """What dsmgp_memory's `needed` is for the table when both sharing claims are kept (build_plan: the arenas of the fit): per
    factor owner npad^2 doubles of factor and nb 128^2 of Dinv -- a COPY leaf owns none --, per leaf 4 npad of vectors and npad D of
    gathered inputs."""
    npad = (t.n + 127) // 128 * 128
    owner = t.op != COPY
    return int(8 * (np.sum(npad[owner] ** 2) + np.sum(npad[owner] // 128 * 128 * 128) + np.sum(4 * npad) + np.sum(npad * D)))


# ---------------------------------------------------------------------------------------------- the wraps a wrong library makes

def wrap_mod(period):
    return lambda l: l % period


def wrap_sub(l):
    return np.where(l >= CHUNK, l - CHUNK, l)


WRAPS = {"l mod 32768": (wrap_mod(CHUNK), CHUNK), "l mod 65536": (wrap_mod(2 * CHUNK), 2 * CHUNK), "l - 32768": (wrap_sub, CHUNK)}


# ---------------------------------------------------------------------------------------------- the longdouble reference

IDX = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))


def _chol(a):
    l11 = np.sqrt(a[0, 0])
    l21, l31 = a[1, 0] / l11, a[2, 0] / l11
    l22 = np.sqrt(a[1, 1] - l21 * l21)
    l32 = (a[2, 1] - l31 * l21) / l22
    l33 = np.sqrt(a[2, 2] - l31 * l31 - l32 * l32)
    return {(0, 0): l11, (1, 0): l21, (1, 1): l22, (2, 0): l31, (2, 1): l32, (2, 2): l33}


def _fwd(c, b):
    z0 = b[0] / c[0, 0]
    z1 = (b[1] - c[1, 0] * z0) / c[1, 1]
    z2 = (b[2] - c[2, 0] * z0 - c[2, 1] * z1) / c[2, 2]
    return [z0, z1, z2]


def _bwd(c, z):
    x2 = z[2] / c[2, 2]
    x1 = (z[1] - c[2, 1] * x2) / c[1, 1]
    x0 = (z[0] - c[1, 0] * x1 - c[2, 0] * x2) / c[0, 0]
    return [x0, x1, x2]


def _inverse(c, S):
    """G = (C C')^-1 as a full symmetric dict: the columns of C^-1 by substitution, then C^-T C^-1."""
    one, zero = np.ones(S, dtype=LD), np.zeros(S, dtype=LD)
    cols = [_fwd(c, [one if i == j else zero for i in range(3)]) for j in range(3)]        # cols[j][k] = (C^-1)_kj
    return {(i, j): sum(cols[i][k] * cols[j][k] for k in range(3)) for i in range(3) for j in range(3)}


def _logdet_half(c):
    return np.log(c[0, 0]) + np.log(c[1, 1]) + np.log(c[2, 2])


def _hyper():
    h = [np.array(v, dtype=np.float64).astype(LD) for v in HYP[:3]]
    return dict(il2_0=np.exp(-2 * h[0][0]), s2_0=np.exp(2 * h[0][1]), sig_0=np.exp(h[0][1]), nz_0=np.exp(2 * h[0][2]),
                il2_1=np.exp(-2 * h[1][:2]), s2_1=np.exp(2 * h[1][2]), nz_1=np.exp(2 * h[1][3]),
                il2_2=np.exp(-2 * h[2][:2]), nz_2=np.exp(2 * h[2][3]))


def _pick(kid, v0, v1, v2):
    return np.where(kid == 0, v0, np.where(kid == 1, v1, v2))


def _kernel(H, kid, a, b, slots=False):
    """k(a, b) per leaf, a and b of shape (S, 2); with `slots` also dk / dtheta_j for the 4 slots of the library's hyper-vector
    (without the noise slot) in the convention of dsmgp_gradients: the true derivatives, times sigma on both IsoSE slots."""
    d0, d1 = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
    r2 = (d0 * d0 + d1 * d1) * H["il2_0"]
    k0 = H["s2_0"] * np.exp(-r2 / 2)
    q0, q1 = d0 * d0 * H["il2_1"][0], d1 * d1 * H["il2_1"][1]
    k1 = H["s2_1"] * np.exp(-(q0 + q1) / 2)
    p0, p1 = a[:, 0] * b[:, 0] * H["il2_2"][0], a[:, 1] * b[:, 1] * H["il2_2"][1]
    k = _pick(kid, k0, k1, p0 + p1)
    if not slots:
        return k
    zero = np.zeros_like(k)
    return k, [_pick(kid, H["sig_0"] * k0 * r2, k1 * q0, -2 * p0), _pick(kid, H["sig_0"] * 2 * k0, k1 * q1, -2 * p1),
               _pick(kid, zero, 2 * k1, zero)]


def reference(t, leaves=None, train_wrap=None, test_wrap=None, target_wrap=None):
    """Every result of the leaves `leaves` (default: all of up to 3 rows) of table `t`, as np.longdouble arrays over the leaf
    axis; per-row results are (S, 3) with NaN where the leaf has no such row, per-test-row results (R, NT) over the routed ones
    of `leaves` (`routed`: their positions in `leaves`)."""
    sel = t.small if leaves is None else np.asarray(leaves, dtype=np.int64)
    S = sel.size
    assert np.all(t.n[sel] <= 3) and np.all(t.kid[sel] < 3)
    n, kid = t.n[sel], t.kid[sel]
    m = [n > i for i in range(3)]
    H = _hyper()
    nan = LD("nan")

    def rows_of(wrap):
        start = t.obs_ptr[sel if wrap is None else wrap(sel)]
        return [t.obs_idx[(start + i) % t.obs_idx.size] for i in range(3)]

    rows = rows_of(train_wrap)
    trows = rows_of(target_wrap)          # (targets_gather_kernel reads the lists on its own: a wrapped gather_leaf does not move it)
    x = [t.X[rows[i]].astype(LD) for i in range(3)]
    y = [t.y[rows[i]].astype(LD) for i in range(3)]
    mean = t.mean[sel].astype(LD)
    noise = _pick(kid, H["nz_0"], H["nz_1"], H["nz_2"]) * np.ones(S, dtype=LD)
    one, zero = np.ones(S, dtype=LD), np.zeros(S, dtype=LD)
    # K_y, padded with an identity block, and its derivatives (4 slots; the noise slot: 2 noise I, the jitter is no parameter)
    A, dA, kss = {}, [dict() for _ in range(STRIDE)], []
    nslot = np.where(kid == 0, 2, 3)                       # the slot of logNoise
    for (i, j) in IDX:
        k, dk = _kernel(H, kid, x[i], x[j], slots=True)
        both = m[i] & m[j]
        if i == j:
            kss.append(np.where(m[i], k, nan))
            A[i, j] = np.where(m[i], k + noise + LD(JITTER), one)
        else:
            A[i, j] = np.where(both, k, zero)
        dk = dk + [zero]
        for s in range(STRIDE):
            v = dk[s] + (np.where(nslot == s, 2 * noise, zero) if i == j else zero)
            dA[s][i, j] = np.where(both, v, zero)
    C = _chol(A)
    G = _inverse(C, S)
    half = _logdet_half(C)
    nl = n.astype(LD)

    def solve(yc):
        z = _fwd(C, yc)
        return z, _bwd(C, z), -(sum(v * v for v in z) + 2 * half + LOG2PI_LD * nl) / 2

    def loo(yv, al):
        mu = [np.where(m[i], yv[i] - al[i] / G[i, i], nan) for i in range(3)]
        var = [np.where(m[i], 1 / G[i, i], nan) for i in range(3)]
        lpd = sum(np.where(m[i], -(LOG2PI_LD - np.log(G[i, i]) + al[i] * al[i] / G[i, i]) / 2, zero) for i in range(3))
        return mu, var, lpd

    out = dict(leaves=sel, n=n, kid=kid, rows=np.stack(rows, axis=1), mask=np.stack(m, axis=1), noise=noise,
               kss=np.stack(kss, axis=1), half_logdet=half)
    out["Ky"] = np.stack([np.stack([A[max(i, j), min(i, j)] for j in range(3)], axis=1) for i in range(3)], axis=1)   # (S, 3, 3), padded
    yc = [np.where(m[i], y[i] - mean, zero) for i in range(3)]
    z, al, mll = solve(yc)
    out["mll"], out["z"] = mll, np.stack(z, axis=1)
    out["alpha"] = np.stack([np.where(m[i], al[i], nan) for i in range(3)], axis=1)
    g = []
    for s in range(STRIDE):
        acc = zero
        for (i, j) in IDX:
            acc = acc + (1 if i == j else 2) * (al[i] * al[j] - G[i, j]) * dA[s][i, j]
        g.append(acc / 2)
    out["grad"] = np.stack(g, axis=1)
    mu, var, lpd = loo(y, al)
    out["loo_mu"], out["loo_var"], out["loo_lpd"] = np.stack(mu, axis=1), np.stack(var, axis=1), lpd
    # k-fold, K = 2 on label = row % 2: G_FF embedded in an identity (the rows outside the fold), factorised by the same code
    kmu, kvar = np.full((S, 3), nan, dtype=LD), np.full((S, 3), nan, dtype=LD)
    klpd, kabs = np.zeros((S, KFOLDS), dtype=LD), np.zeros((S, KFOLDS), dtype=LD)
    lab = [np.where(m[i], t.fold[rows[i]], -1) for i in range(3)]
    for f in range(KFOLDS):
        inF = [lab[i] == f for i in range(3)]
        M = {(i, j): (np.where(inF[i], G[i, i], one) if i == j else np.where(inF[i] & inF[j], G[i, j], zero)) for (i, j) in IDX}
        Cf = _chol(M)
        w = _fwd(Cf, [np.where(inF[i], al[i], zero) for i in range(3)])
        u = _bwd(Cf, w)
        Mi = _inverse(Cf, S)
        cnt = sum(v.astype(np.int64) for v in inF).astype(LD)
        ww, hl = sum(v * v for v in w), _logdet_half(Cf)
        klpd[:, f] = np.where(cnt > 0, -ww / 2 + hl - cnt * LOG2PI_LD / 2, zero)
        kabs[:, f] = ww / 2 + sum(np.abs(np.log(Cf[i, i])) for i in range(3)) + cnt * LOG2PI_LD / 2
        for i in range(3):
            kmu[:, i] = np.where(inF[i], y[i] - u[i], kmu[:, i])
            kvar[:, i] = np.where(inF[i], Mi[i, i], kvar[:, i])
    out["kfold_mu"], out["kfold_var"], out["kfold_lpd"], out["kfold_abs"], out["labels"] = kmu, kvar, klpd, kabs, np.stack(lab, axis=1)
    # the target columns
    tm, tz, tmu, tlpd, tal = [], [], [], [], []
    for q in range(Q):
        yq = [t.Y[trows[i], q].astype(LD) for i in range(3)]
        zq, aq, mq = solve([np.where(m[i], yq[i] - t.Ymean[sel, q].astype(LD), zero) for i in range(3)])
        lm, _, ll = loo(yq, aq)
        tm.append(mq), tz.append(np.stack(zq, axis=1)), tmu.append(np.stack(lm, axis=1)), tlpd.append(ll)
        tal.append(np.stack(aq, axis=1))
    out["targets_mll"], out["targets_z"] = np.stack(tm, axis=1), np.stack(tz, axis=2)                 # (S, Q), (S, 3, Q)
    out["targets_loo_mu"], out["targets_loo_lpd"] = np.stack(tmu, axis=2), np.stack(tlpd, axis=1)
    out["targets_y"] = np.stack([t.Y[trows[i]] for i in range(3)], axis=1)                             # (S, 3, Q)
    # predictions of the routed leaves
    R = np.flatnonzero(t.nt[sel] > 0)
    out["routed"] = R
    pm, pv, pk = np.empty((R.size, NT), dtype=LD), np.empty((R.size, NT), dtype=LD), np.empty((R.size, NT), dtype=LD)
    rstart = t.route_ptr[sel[R] if test_wrap is None else test_wrap(sel[R])]
    CR = {k: v[R] for k, v in C.items()}
    for j in range(NT):
        xt = t.Xt[t.route_idx[(rstart + j) % t.route_idx.size]].astype(LD)
        kt = [np.where(m[i][R], _kernel(H, kid[R], xt, x[i][R]), zero[R]) for i in range(3)]
        v = _fwd(CR, kt)
        pk[:, j] = _kernel(H, kid[R], xt, xt)
        pm[:, j] = mean[R] + sum(kt[i] * np.where(m[i][R], al[i][R], zero[R]) for i in range(3))
        pv[:, j] = pk[:, j] - sum(u * u for u in v) + noise[R]
    out["pred_mu"], out["pred_var"], out["pred_kss"] = pm, pv, pk
    return out


# ---------------------------------------------------------------------------------------------- tolerances over the leaf axis

def _f(a):
    return np.asarray(a, dtype=np.float64)


def tolerances(t, ref):
    """The project's tolerances at the reference values `ref`, once (the reference does not round at float64): for every key of
    `ref` that the device returns, an array of its shape.
        mll                  pred_tolerance.mll_tol;   alpha: pred_tolerance.alpha_tol
        grad                 tests/test_gradients_gpu.py::_tolerance: max(1e-13, 64 cond eps max(1, |g|_inf)) per leaf
        loo_*, targets_loo_* loo_dense.loo_tol (moment_tol carried through the density, plus the rounding of the leaf's sum)
        kfold_mu / _var      kfold_dense.moment_tols;  kfold_lpd: kfold_dense.lpd_tol_backward (the factor's backward error,
                             once: one side rounds) plus kfold_dense.lpd_floor (the float64 sum of the density's terms)
        targets_z / _mll     targets_dense.z_tol, mll_tol;   pred_*: pred_tolerance.moment_tol"""
    S = ref["leaves"].size
    mask, n = ref["mask"], ref["n"]
    # cond_2(K_y) and |K_y|_2 of the leaf's own block (float64 eigenvalues: the tolerance's side, not the reference's)
    H = _hyper()
    x = [t.X[ref["rows"][:, i]].astype(LD) for i in range(3)]
    Ky = np.zeros((S, 3, 3))
    for (i, j) in IDX:
        k = _f(_kernel(H, ref["kid"], x[i], x[j]))
        both = mask[:, i] & mask[:, j]
        Ky[:, i, j] = Ky[:, j, i] = np.where(both, k + (_f(ref["noise"]) + JITTER if i == j else 0.0), 1.0 if i == j else 0.0)
    cond, normK = np.empty(S), np.empty(S)
    for k in (1, 2, 3):                                     # the leaf's own block: the padding's eigenvalue 1 is not K_y's
        w = np.flatnonzero(n == k)
        e = np.linalg.eigvalsh(Ky[w][:, :k, :k])
        cond[w], normK[w] = e[:, -1] / e[:, 0], e[:, -1]
    noise, kss = _f(ref["noise"]), _f(ref["kss"])
    tol = dict(cond=cond)
    tol["mll"] = np.maximum(1e-13, 64.0 * cond * EPS * np.maximum(1.0, np.abs(_f(ref["mll"]))))
    amax = np.nanmax(np.abs(_f(ref["alpha"])), axis=1)
    tol["alpha"] = np.broadcast_to(np.maximum(1e-13, 64.0 * cond * EPS * amax)[:, None], (S, 3))
    gmax = np.max(np.abs(_f(ref["grad"])), axis=1)
    tol["grad"] = np.broadcast_to(np.maximum(1e-13, 64.0 * cond * EPS * np.maximum(1.0, gmax))[:, None], (S, STRIDE))

    def loo_tol(yv, mu, var):
        yscale = np.maximum(1.0, np.nanmax(np.abs(np.where(mask, yv, np.nan)), axis=1))
        tm = RTOL * np.abs(mu) + ATOL * yscale[:, None]
        tv = RTOL * np.abs(var) + ATOL * np.maximum(1.0, kss + noise[:, None])
        d = yv - mu                                        # pred_tolerance.Prop through loo_dense.lpd_terms
        e_dd = 2.0 * np.abs(d) * tm
        e = 0.5 * (tv / np.abs(var) + e_dd / np.abs(var) + d * d * tv / (var * var))
        terms = -0.5 * (np.log(var) + d * d / var + float(LOG2PI_LD))
        ts = np.nansum(e, axis=1) + (8 + n / 256.0) * EPS * np.nanmean(np.abs(terms), axis=1)
        return tm, tv, ts

    yv = np.where(mask, t.y[ref["rows"]], np.nan)
    tol["loo_mu"], tol["loo_var"], tol["loo_lpd"] = loo_tol(yv, _f(ref["loo_mu"]), _f(ref["loo_var"]))
    tq = [loo_tol(np.where(mask, ref["targets_y"][:, :, q], np.nan), _f(ref["targets_loo_mu"][:, :, q]), _f(ref["loo_var"]))
          for q in range(Q)]
    tol["targets_loo_mu"] = np.stack([v[0] for v in tq], axis=2)
    tol["targets_loo_lpd"] = np.stack([v[2] for v in tq], axis=1)
    yscale = np.maximum(1.0, np.nanmax(np.abs(yv), axis=1))
    tol["kfold_mu"] = RTOL * np.abs(_f(ref["kfold_mu"])) + ATOL * yscale[:, None]
    tol["kfold_var"] = RTOL * np.abs(_f(ref["kfold_var"])) + ATOL * np.maximum(1.0, kss + noise[:, None])
    a2 = np.nansum(_f(ref["alpha"]) ** 2, axis=1)
    cnt = np.stack([np.sum(ref["labels"] == f, axis=1) for f in range(KFOLDS)], axis=1)
    tol["kfold_lpd"] = (n * EPS * (a2 * normK + n * cond))[:, None] + (8.0 + cnt / 256.0) * EPS * _f(ref["kfold_abs"])
    Z = _f(ref["targets_z"])
    zt = np.maximum(1e-13, 64.0 * cond[:, None] * EPS * np.max(np.abs(Z), axis=1))                     # (S, Q)
    tol["targets_z"] = np.broadcast_to(zt[:, None, :], Z.shape)
    tol["targets_mll"] = np.sum(np.abs(Z), axis=1) * zt + np.maximum(1e-13, 64.0 * cond * EPS * np.maximum(
        1.0, np.abs(_f(ref["half_logdet"]))))[:, None]
    R = ref["routed"]
    tol["pred_mu"] = RTOL * np.abs(_f(ref["pred_mu"])) + ATOL * yscale[R][:, None]
    tol["pred_var"] = RTOL * np.abs(_f(ref["pred_var"])) + ATOL * np.maximum(1.0, _f(ref["pred_kss"]) + noise[R][:, None])
    return tol


# ---------------------------------------------------------------------------------------------- where the device puts things

def device_view(t, ref, res):
    """The device's results `res` (mll, grad, loo = (mu, var, lpd), kfold = (mu, var, lpd, info), targets_mll, targets_loo =
    (mu, var, lpd), pred = (mu, var); any subset) in the layout of `reference`: key -> float64 array."""
    sel, mask = ref["leaves"], ref["mask"]
    pos = np.minimum(t.obs_ptr[sel][:, None] + np.arange(3)[None, :], t.obs_idx.size - 1)

    def per_row(v):
        return np.where(mask, np.asarray(v)[pos], np.nan)

    out = {}
    if "mll" in res:
        out["mll"] = res["mll"][sel]
    if "grad" in res:
        out["grad"] = res["grad"][sel][:, :STRIDE]
    if "loo" in res:
        out["loo_mu"], out["loo_var"], out["loo_lpd"] = per_row(res["loo"][0]), per_row(res["loo"][1]), res["loo"][2][sel]
    if "kfold" in res:
        out["kfold_mu"], out["kfold_var"], out["kfold_lpd"] = per_row(res["kfold"][0]), per_row(res["kfold"][1]), res["kfold"][2][sel]
    if "targets_mll" in res:
        out["targets_mll"] = res["targets_mll"][sel]
    if "targets_loo" in res:
        mu = np.asarray(res["targets_loo"][0])
        out["targets_loo_mu"] = np.where(mask[:, :, None], mu[pos], np.nan)
        out["targets_loo_lpd"] = res["targets_loo"][2][sel]
    if "pred" in res:
        e = t.route_ptr[sel[ref["routed"]]][:, None] + np.arange(NT)[None, :]
        out["pred_mu"], out["pred_var"] = np.asarray(res["pred"][0])[e], np.asarray(res["pred"][1])[e]
    return out


def compare(got, ref, tol, keys=None):
    """Worst |got - ref| / tol per key over all entries (NaN = no such row on both sides), and where."""
    worst = {}
    for k in (got if keys is None else keys):
        g, r, tl = np.asarray(got[k]), ref[k], np.asarray(tol[k])
        assert g.shape == r.shape == tl.shape, (k, g.shape, r.shape, tl.shape)
        nan = np.isnan(_f(r))
        assert np.array_equal(np.isnan(g), nan), (k, "NaN pattern")
        ratio = np.where(nan, 0.0, _f(np.abs(g.astype(LD) - r)) / tl)
        w = int(np.argmax(ratio))
        worst[k] = (float(ratio.flat[w]), int(ref["leaves"][np.unravel_index(w, ratio.shape)[0]]) if k not in ("pred_mu", "pred_var")
                    else int(ref["leaves"][ref["routed"][np.unravel_index(w, ratio.shape)[0]]]))
    return worst


# ---------------------------------------------------------------------------------------------- the larger leaves, float64

def large_leaf(t, l):
    """The float64 dense reference of one larger leaf (tests/dense_gp.py and the helpers the other suites use): values, and the
    tolerances of those suites: the log marginal, alpha, the gradient and the predictive moments once (as tests/test_matern_gpu.py
    and test_rq_gpu.py use them against float64 dense references), LOO, k-fold and the targets doubled (as tests/test_loo_gpu.py,
    test_kfold_gpu.py and test_targets_gpu.py double them where both sides round at float64)."""
    import dense_gp
    import kfold_dense as kd
    import loo_dense
    import targets_dense as td
    from pred_tolerance import alpha_tol, mll_tol, moment_tol
    rows = t.obs_idx[t.obs_ptr[l]:t.obs_ptr[l + 1]]
    kind, hyp = KINDS[t.kid[l]], np.array(HYP[t.kid[l]])
    X, y, mean = t.X[rows], t.y[rows], float(t.mean[l])
    gp = dense_gp.DenseGP(kind, hyp, X, y, mean)
    assert gp.info == 0
    cond, noise = gp.cond, gp.noise
    kss = np.diag(gp.K)
    r = dict(rows=rows, cond=cond, F=gp.F)
    r["mll"] = (gp.mll(), float(mll_tol(gp.mll(), cond)))
    r["alpha"] = (gp.alpha, alpha_tol(gp.alpha, cond))
    g = gp.grad()
    r["grad"] = (g, max(1e-13, 64.0 * cond * EPS * max(1.0, float(np.max(np.abs(g))))))
    lm, lv, ll = loo_dense.loo_from_factor(gp.F, y, mean)
    tm, tv, _, ts = loo_dense.loo_tol(y, lm, lv, kss, noise)
    r["loo"] = (lm, lv, float(np.sum(ll)), 2.0 * tm, 2.0 * tv, 2.0 * ts)
    km, kv, kl = kd.kfold_from_factor(gp.F, y, mean, t.fold[rows], KFOLDS)
    ktm, ktv = kd.moment_tols(y, km, kv, kss, noise)
    _, normK = kd.factor_stats(gp.F)
    r["kfold"] = (km, kv, kl, 2.0 * ktm, 2.0 * ktv, 2.0 * kd.lpd_tol_backward(y.size, cond, gp.alpha, normK))
    Yl = t.Y[rows]
    Z, tmll, _ = td.reference(gp.F, Yl, t.Ymean[l])
    r["targets"] = (Z, tmll, 2.0 * td.z_tol(Z, cond), 2.0 * td.mll_tol(Z, gp.F, cond))
    tl = [loo_dense.loo_from_factor(gp.F, Yl[:, q], float(t.Ymean[l, q])) for q in range(Q)]
    tt = [loo_dense.loo_tol(Yl[:, q], tl[q][0], tl[q][1], kss, noise) for q in range(Q)]
    r["targets_loo"] = (np.stack([v[0] for v in tl], axis=1), np.array([np.sum(v[2]) for v in tl]),
                        2.0 * np.stack([v[0] for v in tt], axis=1), 2.0 * np.array([v[3] for v in tt]))
    if t.nt[l]:
        xt = t.Xt[t.route_idx[t.route_ptr[l]:t.route_ptr[l + 1]]]
        pm, pv = gp.prediction(xt)
        import dense_kernels as dk
        ptm, ptv = moment_tol(pm, pv, dk.prior_diag(kind, hyp[:-1], xt), noise, max(1.0, float(np.max(np.abs(y)))))
        r["pred"] = (pm, pv, ptm, ptv)
    return r
