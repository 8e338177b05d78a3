"""Generate tests/golden/gp_targets_grad.npz: 50-digit hyper-parameter gradients of the per-column log marginal likelihoods of
several target columns on one factorisation (dsmgp_mll_columns_gradients).

For a single leaf with inputs X, targets Y (n x Q), per-column means m and K_y = K + (noise + 1e-8) I, every case is evaluated
in mpmath at 50 digits straight from the textbook equation
    d mll_j / d theta = 0.5 tr((alpha_j alpha_j^T - G) dK_y / d theta),   G = K_y^-1,   alpha_j = G (y_j - m_j),
entry by entry on K_y^-1 = L^-T L^-1 -- never through A = L^-T Z, the rank-Q update of the contraction or the trace identity
tr(P K) = (y.alpha - c alpha.alpha) - (n - c tr G) the device uses.  The components are stored in the library's convention
(include/dsmgp_hip.h at dsmgp_gradients; tests/targets_grad_dense.py restates it): [dl..., ds, dnoise], [dl..., da, ds, dnoise]
for the rational quadratic kinds, the factor sigma of IsoSE / ArdSE's variance slot, ArdSE dl = 0 with the true d/dlog l_d stored
as `grad_true`, the dummy slots of the linear kinds.

Per case: X, Y, mean, hyp (the library hyper-vector including logNoise), grad (Q x len(hyp): one row per column), w (the fixed
signed weight vector targets_grad_dense.signed_weights(Q)), wsum (sum_j w_j grad[j] at 50 digits), mll (Q), cond = cond_2(K_y)
(4 digits: tolerance metadata), and n, c_trKinv, weak for the weak-signal floor of the tolerance.  Cases: all eleven kernel
kinds; n in {1, 2, 128, 130, 300}; Q in {1, 3, 16, 17, 33}; D in {1, 3}; a column with an offset of 1000, a column of noise, a
zero weight; one weak-signal IsoSE case (sigma^2 / c = 1e-8).  Before anything is stored the float64 dense restatement
(tests/targets_grad_dense.py) must agree with the 50 digits within its own tolerance.  Imports numpy, scipy and mpmath, the
data generators of make_pred_golden.py and tests/targets_grad_dense.py.  Run from the repo root:
    python tests/golden/make_targets_grad_golden.py     (the cases run in parallel processes; a few minutes; byte-reproducible)
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_pred_golden import uniform, normal  # noqa: E402
import mp_kernels as mpk  # noqa: E402
import targets_grad_dense as tgd  # noqa: E402

mp.mp.dps = 50
JIT = mp.mpf("1e-8")


def mp_case(kind, hyp, X, Y, mean):
    """(grad[Q][len(hyp)], mll[Q], K_y rounded, c tr K_y^-1) at 50 digits."""
    n, D = X.shape
    Q = Y.shape[1]
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    h = [mp.mpf(float(v)) for v in hyp[:-1]]
    noise = mp.e ** (2 * mp.mpf(float(hyp[-1])))
    c = noise + JIT
    nt = len(hyp) - 1
    par = mpk.unpack(kind, h, D)
    K = []
    dK = [[] for _ in range(nt)]
    for i in range(n):
        row, drow = [], [[] for _ in range(nt)]
        for j in range(i + 1):
            k, dk = mpk.d_hyper(kind, x[i], x[j], *par)
            dk = mpk.mll_convention(kind, h, dk)
            row.append(k)
            for t in range(nt):
                drow[t].append(dk[t])
        K.append(row)
        for t in range(nt):
            dK[t].append(drow[t])
    L = []
    for i in range(n):
        row = []
        for j in range(i):
            row.append((K[i][j] - mp.fdot(row[:j], L[j][:j])) / L[j][j])
        row.append(mp.sqrt(K[i][i] + c - mp.fdot(row, row)))
        L.append(row)
    col = []                                                    # columns of L^-1: col[j][k - j] = (L^-1)[k][j]
    for j in range(n):
        cj = [1 / L[j][j]]
        for i in range(j + 1, n):
            cj.append(-mp.fdot(L[i][j:i], cj) / L[i][i])
        col.append(cj)
    Kinv = [[mp.fdot(col[i], col[j][i - j:]) for j in range(i + 1)] for i in range(n)]
    trG = mp.fsum(Kinv[i][i] for i in range(n))
    # tr(G dK_t): lower triangles, off-diagonal entries twice
    trGdK = [mp.fsum(2 * mp.fdot(Kinv[i][:i], dK[t][i][:i]) + Kinv[i][i] * dK[t][i][i] for i in range(n)) for t in range(nt)]
    logdet = 2 * mp.fsum(mp.log(L[i][i]) for i in range(n))
    grad, mll = [], []
    for j in range(Q):
        yc = [mp.mpf(float(Y[i, j])) - mp.mpf(float(mean[j])) for i in range(n)]
        al = [mp.fdot(Kinv[i], yc[:i + 1]) + mp.fsum(Kinv[k][i] * yc[k] for k in range(i + 1, n)) for i in range(n)]
        g = []
        for t in range(nt):
            quad = mp.fsum(al[i] * (2 * mp.fdot(dK[t][i][:i], al[:i]) + dK[t][i][i] * al[i]) for i in range(n))
            g.append((quad - trGdK[t]) / 2)
        g.append(noise * (mp.fdot(al, al) - trG))               # 0.5 tr(P dK_y / dlog sigma_n), dK_y = 2 noise I
        grad.append(g)
        mll.append(-(mp.fdot(yc, al) + logdet + n * mp.log(2 * mp.pi)) / 2)
    Kyf = np.array([[float(K[max(i, j)][min(i, j)] + (c if i == j else 0)) for j in range(n)] for i in range(n)])
    return grad, mll, Kyf, c * trG


def _logl(D):
    return list(np.log(np.linspace(0.5, 0.9, D)))


LN = np.log(0.2)
# name, kind, n, D, Q, hyp without the noise, logNoise, weak
SPECS = [
    ("isose_n1_q1", 0, 1, 1, 1, [np.log(0.5), 0.1], LN, False),
    ("isolinear_n1_q3", 2, 1, 3, 3, [np.log(0.8), 0.0], LN, False),
    ("isose_n2_q3", 0, 2, 1, 3, [np.log(0.6), -0.2], LN, False),
    ("ardmatern32_n2_q16", 7, 2, 3, 16, _logl(3) + [0.1], LN, False),
    ("isose_n128_q16", 0, 128, 3, 16, [np.log(0.4), 0.0], LN, False),
    ("ardse_n130_q17", 1, 130, 3, 17, list(np.log([0.4, 0.6, 0.9])) + [-0.3], LN, False),
    ("isolinear_n130_q3", 2, 130, 3, 3, [np.log(1.0), 0.0], LN, False),
    ("ardlinear_n130_q17", 3, 130, 3, 17, list(np.log([0.8, 1.2, 1.6])) + [0.0], LN, False),
    ("ardseproduct_n130_q33", 4, 130, 3, 33, _logl(3) + [0.0], LN, False),
    ("isomatern32_n128_q1", 5, 128, 1, 1, [np.log(0.5), 0.0], LN, False),
    ("isomatern52_n130_q3", 6, 130, 3, 3, [np.log(0.7), 0.2], LN, False),
    ("ardmatern32_n130_q17", 7, 130, 3, 17, _logl(3) + [0.1], LN, False),
    ("ardmatern52_n300_q3", 8, 300, 3, 3, _logl(3) + [-0.1], np.log(0.25), False),
    ("isorq_n130_q16", 9, 130, 1, 16, [np.log(0.5), np.log(2.0), 0.0], LN, False),
    ("ardrq_n300_q3", 10, 300, 3, 3, _logl(3) + [np.log(0.3), -0.1], np.log(0.25), False),
    ("isose_n300_q33", 0, 300, 3, 33, [np.log(0.4), 0.0], LN, False),
    ("ardlinear_n300_q1", 3, 300, 1, 1, [np.log(1.2), 0.0], LN, False),
    # weak signal: sigma^2 / c = 1e-8, data at noise level (the floor of the host's trace identity)
    ("isose_weak_n130_q3", 0, 130, 1, 3, [np.log(0.4), 0.5 * np.log(1e-8 * (0.04 + 1e-8))], LN, True),
]


def targets(si, X, Q, weak):
    n = X.shape[0]
    cols = []
    for j in range(Q):
        e = normal(5200 + 40 * si + j, 0, n)
        if weak:
            cols.append(0.2 * e)
        elif j % 5 == 4:
            cols.append(e)                                           # a column of noise
        else:
            f = np.sin((2.0 + j % 4) * X[:, 0]) * np.cos(0.5 * j * X[:, -1]) + 0.1 * e
            cols.append(f + (1000.0 if j == 1 else 0.0))             # one column with an offset
    return np.stack(cols, axis=1)


def run_case(args):
    si, (name, kind, n, D, Q, h, logNoise, weak) = args
    X = uniform(5000 + si, 0, n * D).reshape((n, D), order="F")
    Y = targets(si, X, Q, weak)
    mean = np.mean(Y, axis=0) if n > 2 else np.zeros(Q)              # n = 1: y - mean(y) would be zero
    hyp = np.array(list(h) + [logNoise], dtype=np.float64)
    grad, mll, Ky, ctr = mp_case(kind, hyp, X, Y, mean)
    ev = np.linalg.eigvalsh(Ky)
    cond = float(f"{ev[-1] / ev[0]:.4g}")
    w = tgd.signed_weights(Q)
    lib = [list(g) for g in grad]
    rec = {}
    if kind == 1:
        rec["grad_true"] = np.array([[float(v) for v in g[:D]] for g in grad])
        rec["wsum_true"] = np.array([float(mp.fsum(mp.mpf(float(w[j])) * grad[j][t] for j in range(Q))) for t in range(D)])
        for g in lib:
            g[:D] = [mp.mpf(0)] * D
    G = np.array([[float(v) for v in g] for g in lib])
    wsum = np.array([float(mp.fsum(mp.mpf(float(w[j])) * lib[j][t] for j in range(Q))) for t in range(len(hyp))])
    # the float64 dense restatement must agree with the 50 digits before anything is stored
    worst = 0.0
    for ard_true in ((False, True) if kind == 1 else (False,)):
        Gd, mlld, _ = tgd.column_gradients(kind, hyp, X, Y, mean, ard_true=ard_true)
        Gr = G.copy()
        if ard_true:
            Gr[:, :D] = rec["grad_true"]
        tol = tgd.tolerance(Gr, w, cond, kind, hyp, weak, n, float(ctr))
        r = float(np.max(np.abs(tgd.weighted(Gd, w) - tgd.weighted(Gr, w)) / tol))
        for j in range(Q):
            one = np.zeros(Q)
            one[j] = 1.0
            r = max(r, float(np.max(np.abs(Gd[j] - Gr[j]) / tgd.tolerance(Gr, one, cond, kind, hyp, weak, n, float(ctr)))))
        worst = max(worst, r)
        assert r <= 1.0, (name, ard_true, r)
    mllf = np.array([float(v) for v in mll])
    assert np.max(np.abs(mlld - mllf)) <= 64.0 * cond * tgd.EPS * max(1.0, float(np.max(np.abs(mllf)))), name
    rec.update(kind=kind, X=X, Y=Y, mean=mean, hyp=hyp, grad=G, w=w, wsum=wsum, mll=mllf, cond=cond, n=n, c_trKinv=float(ctr),
               weak=weak)
    print(f"{name:24s} kind {kind:2d} n {n:3d} D {D} Q {Q:2d}  cond {cond:9.4g}  |g|inf {np.max(np.abs(G)):9.3g}  "
          f"dense err / tol {worst:.2g}", flush=True)
    return name, rec


def main():
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        results = pool.map(run_case, list(enumerate(SPECS)), chunksize=1)
    flat = {}
    for name, rec in results:
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
    out = os.path.join(HERE, "gp_targets_grad.npz")
    mpk.savez_reproducible(out, flat, compresslevel=9)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
