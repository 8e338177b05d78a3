"""Generate tests/golden/gp_loo_columns.npz: 50-digit leave-one-out moments, densities and hyper-parameter gradients of several
target columns on one factorisation (dsmgp_loo_columns, dsmgp_loo_columns_gradients).

For a single leaf with inputs X, targets Y (n x Q), per-column means m and K_y = K + (noise + 1e-8) I everything is evaluated
in mpmath at 50 digits from G = K_y^-1 (mpmath's own inverse): the moments of GPML eqs. 5.10-5.12 per column and eq. 5.13 as
printed, column by column -- never through the M form, H, U or the trace identities the device uses.  Every gradient component
is the true derivative (tests/loo_columns_dense.py states the convention).  Before anything is stored
  * the weighted gradient sum_q c_q dlpd_q/dtheta must agree with a central difference (step 1e-20, 50 digits) of
    sum_q c_q lpd_q in every component, and
  * both float64 forms of tests/loo_columns_dense.py must agree with the 50 digits within the module's own tolerances.

Per case: kind, X, Y, mean, hyp (including logNoise), mu (n x Q), var (n), lpd (Q), grad (Q x len(hyp), one row per column),
w (loo_columns_dense.weights(Q): non-negative, a zero weight when Q = 3), wsum (sum_q w_q grad[q] at 50 digits), kss
(k(x_i, x_i)), cond = cond_2(K_y) (4 digits: tolerance metadata), n, weak.  Cases: all eleven kernel kinds, n <= 40,
Q in {1, 3}, one weak-signal IsoLinear case (1 / l^2 = 1e-8 c).  Imports numpy, scipy and mpmath, the generators of
make_pred_golden.py, the kernel entries of make_targets_grad_golden.py and tests/loo_columns_dense.py.  Run from the repo root:
    python tests/golden/make_loo_columns_golden.py      (parallel processes; about a minute; byte-reproducible)
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
import loo_columns_dense as lcd  # noqa: E402

mp.mp.dps = 50
JIT = mp.mpf("1e-8")


def inverse_parts(kind, hmp, x, noise_log):
    """(G, d, K, [dK_y per theta incl. the noise]) at 50 digits for the hyper-vector hmp (mp numbers, without the noise)."""
    n = len(x)
    nt = len(hmp)
    noise = mp.e ** (2 * noise_log)
    par = mpk.unpack(kind, hmp, len(x[0]))
    K = mp.zeros(n, n)
    dK = [mp.zeros(n, n) for _ in range(nt + 1)]
    for i in range(n):
        for j in range(i + 1):
            k, dk = mpk.d_hyper(kind, x[i], x[j], *par)
            K[i, j] = K[j, i] = k
            for t in range(nt):
                dK[t][i, j] = dK[t][j, i] = dk[t]
        dK[nt][i, i] = 2 * noise
    Ky = K + (noise + JIT) * mp.eye(n)
    G = mp.inverse(Ky)
    G = (G + G.T) / 2
    return G, [G[i, i] for i in range(n)], K, dK


def lpd_columns(G, d, Yc):
    """(A = G Yc, lpd per column)."""
    n, Q = Yc.rows, Yc.cols
    A = G * Yc
    log2pi = mp.log(2 * mp.pi)
    return A, [mp.fsum(-(log2pi - mp.log(d[i]) + A[i, q] ** 2 / d[i]) / 2 for i in range(n)) for q in range(Q)]


def mp_case(kind, hyp, X, Y, mean, w):
    n, D = X.shape
    Q = Y.shape[1]
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    h = [mp.mpf(float(v)) for v in hyp[:-1]]
    ln = mp.mpf(float(hyp[-1]))
    Yc = mp.matrix(n, Q)
    for i in range(n):
        for q in range(Q):
            Yc[i, q] = mp.mpf(float(Y[i, q])) - mp.mpf(float(mean[q]))
    G, d, K, dK = inverse_parts(kind, h, x, ln)
    A, lpd = lpd_columns(G, d, Yc)
    mu = [[mp.mpf(float(Y[i, q])) - A[i, q] / d[i] for q in range(Q)] for i in range(n)]
    grad = [[None] * len(hyp) for _ in range(Q)]
    for t, dKt in enumerate(dK):
        Z = G * dKt
        ZG = Z * G
        ZA = Z * A
        for q in range(Q):
            grad[q][t] = mp.fsum((A[i, q] * ZA[i, q] - (1 + A[i, q] ** 2 / d[i]) * ZG[i, i] / 2) / d[i] for i in range(n))
    wm = [mp.mpf(float(v)) for v in w]
    wsum = [mp.fsum(wm[q] * grad[q][t] for q in range(Q)) for t in range(len(hyp))]
    # self-check: central differences of sum_q c_q lpd_q at 50 digits
    step = mp.mpf("1e-20")
    full = h + [ln]

    def objective(theta):
        Gt, dt, _, _ = inverse_parts(kind, theta[:-1], x, theta[-1])
        return mp.fsum(wq * v for wq, v in zip(wm, lpd_columns(Gt, dt, Yc)[1]))

    for t in range(len(full)):
        up = list(full)
        dn = list(full)
        up[t] += step
        dn[t] -= step
        fd = (objective(up) - objective(dn)) / (2 * step)
        scale = max(1, abs(wsum[t]))
        assert abs(fd - wsum[t]) <= mp.mpf("1e-25") * scale, (kind, t, fd, wsum[t])
    Kyf = np.array([[float(K[i, j] + ((mp.e ** (2 * ln) + JIT) if i == j else 0)) for j in range(n)] for i in range(n)])
    kss = np.array([float(K[i, i]) for i in range(n)])
    return (np.array([[float(v) for v in row] for row in mu]), np.array([float(1 / v) for v in d]), np.array([float(v) for v in lpd]),
            np.array([[float(v) for v in g] for g in grad]), np.array([float(v) for v in wsum]), Kyf, kss)


def _logl(D):
    return list(np.log(np.linspace(0.5, 0.9, D)))


LN = np.log(0.2)
# name, kind, n, D, Q, hyp without the noise, logNoise, weak
SPECS = [
    ("isose_n1_q1", 0, 1, 1, 1, [np.log(0.5), 0.1], LN, False),
    ("isose_n40_q3", 0, 40, 3, 3, [np.log(0.4), 0.0], LN, False),
    ("ardse_n33_q3", 1, 33, 3, 3, list(np.log([0.4, 0.6, 0.9])) + [-0.3], LN, False),
    ("isolinear_n40_q3", 2, 40, 3, 3, [np.log(1.0), 0.0], LN, False),
    ("isolinear_weak_n40_q3", 2, 40, 1, 3, [0.5 * np.log(1.0 / (1e-8 * (0.01 + 1e-8))), 0.0], np.log(0.1), True),
    ("ardlinear_n37_q3", 3, 37, 3, 3, list(np.log([0.8, 1.2, 1.6])) + [0.0], LN, False),
    ("ardseproduct_n40_q1", 4, 40, 3, 1, _logl(3) + [0.0], LN, False),
    ("isomatern32_n40_q3", 5, 40, 1, 3, [np.log(0.5), 0.0], LN, False),
    ("isomatern52_n31_q3", 6, 31, 3, 3, [np.log(0.7), 0.2], LN, False),
    ("ardmatern32_n40_q3", 7, 40, 3, 3, _logl(3) + [0.1], LN, False),
    ("ardmatern52_n40_q1", 8, 40, 3, 1, _logl(3) + [-0.1], np.log(0.25), False),
    ("isorq_n40_q3", 9, 40, 1, 3, [np.log(0.5), np.log(2.0), 0.0], LN, False),
    ("ardrq_n39_q3", 10, 39, 3, 3, _logl(3) + [np.log(0.3), -0.1], np.log(0.25), False),
    ("isose_n2_q3", 0, 2, 1, 3, [np.log(0.6), -0.2], LN, False),
]


def targets(si, X, Q, weak):
    n = X.shape[0]
    cols = []
    for q in range(Q):
        e = normal(6200 + 40 * si + q, 0, n)
        if weak:
            cols.append(0.1 * e)
        else:
            f = np.sin((2.0 + q) * X[:, 0]) * np.cos(0.5 * q * X[:, -1]) + 0.1 * e
            cols.append(f + (50.0 if q == 1 else 0.0))                # one column with an offset
    return np.stack(cols, axis=1)


def run_case(args):
    si, (name, kind, n, D, Q, h, logNoise, weak) = args
    X = uniform(6000 + si, 0, n * D).reshape((n, D), order="F")
    Y = targets(si, X, Q, weak)
    mean = np.mean(Y, axis=0) + 0.05 if n > 2 else np.zeros(Q)       # not the column mean itself: the means are arguments
    hyp = np.array(list(h) + [logNoise], dtype=np.float64)
    w = lcd.weights(Q)
    mu, var, lpd, grad, wsum, Ky, kss = mp_case(kind, hyp, X, Y, mean, w)
    ev = np.linalg.eigvalsh(Ky)
    cond = float(f"{ev[-1] / ev[0]:.4g}")
    rec = dict(kind=kind, X=X, Y=Y, mean=mean, hyp=hyp, mu=mu, var=var, lpd=lpd, grad=grad, w=w, wsum=wsum, kss=kss, cond=cond,
               n=n, weak=weak)
    # the float64 dense restatement, both forms, must agree with the 50 digits before anything is stored
    md, vd, ld_ = lcd.moments(kind, hyp, X, Y, mean)
    worst_m = 0.0
    for q in range(Q):
        tm, tv, _, ts = lcd.moment_tolerances(rec, q)
        worst_m = max(worst_m, float(np.max(np.abs(md[:, q] - mu[:, q]) / tm)), float(np.max(np.abs(vd - var) / tv)),
                      abs(ld_[q] - lpd[q]) / ts)
    tol = lcd.gradient_tolerance(rec, grad, w)
    r_lit = float(np.max(np.abs(lcd.weighted(lcd.column_gradients_literal(kind, hyp, X, Y, mean), w) - wsum) / tol))
    r_m = float(np.max(np.abs(lcd.weighted_gradient(kind, hyp, X, Y, mean, w) - wsum) / tol))
    assert worst_m <= 1.0 and r_lit <= 1.0 and r_m <= 1.0, (name, worst_m, r_lit, r_m)
    print(f"{name:24s} kind {kind:2d} n {n:3d} D {D} Q {Q}  cond {cond:9.4g}  |g|inf {np.max(np.abs(grad)):9.3g}  "
          f"dense err / tol: moments {worst_m:.2g} literal {r_lit:.2g} M {r_m:.2g}", flush=True)
    return name, rec


def main():
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        results = pool.map(run_case, list(enumerate(SPECS)), chunksize=1)
    flat = {}
    for name, rec in results:
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
    out = os.path.join(HERE, "gp_loo_columns.npz")
    mpk.savez_reproducible(out, flat, compresslevel=9)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
