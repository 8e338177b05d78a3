"""Generate tests/golden/gp_loo_grad.npz: 50-digit hyper-parameter gradients of the leave-one-out log predictive density.

lpd = sum_i -(log 2pi - log d_i + alpha_i^2 / d_i) / 2 of one leaf (GPML 5.4.2; d = diag K_y^-1, alpha = K_y^-1 (y - m),
K_y = K + (exp(2 logNoise) + 1e-8) I, the mean m held fixed) and its derivative with respect to every entry of the library
hyper-vector [logl..., logs, logNoise], GPML eq. 5.13 evaluated LITERALLY in mpmath at 50 digits from G = K_y^-1:

    dlpd/dtheta = sum_i (alpha_i [Z alpha]_i - (1 + alpha_i^2 / d_i) [Z G]_ii / 2) / d_i,   Z = G dK_y/dtheta

(not through the matrix M of tests/loo_grad_dense.py, which is what the device and the float64 helper use).  Every component is
also checked against a 50-digit central difference of lpd with step h = 1e-15: the difference's truncation error is
h^2 |lpd'''| / 6 ~ 1e-30 |lpd'''|, and the generator refuses to write when the two differ by more than 1e-24 max(1, |g|).
The dummy variance slot of the linear kinds is 0 by definition (lpd does not depend on it).

Cases: all nine kinds; n in {1, 2, 127, 128, 129, 300}; D in {1, 8, 40} and D = 35 for ArdSE (the staging limit of the
contraction); literal 5.13 costs n^3 multiprecision operations per hyper-parameter, so n = 300 goes with an iso kind and D = 40
with n <= 64.  Means that differ from mean(y) by more than 0.1, targets with max|y| > 500 once, one weak-signal case
(sigma^2 / c = 1e-8) for IsoSE and one for IsoLinear.  Conditions asserted before anything is stored: cond_2(K_y) <= 1e6, and
the float64 dense helper (loo_grad_dense.loo_grad_dense) within 0.05 of loo_grad_dense.tolerance on every component.
Run from the repo root:  python tests/golden/make_loo_grad_golden.py   (the cases run in parallel processes; a few minutes;
the output is byte-reproducible)
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

import dense_kernels  # noqa: E402
import loo_grad_dense as lgd  # noqa: E402
from make_pred_golden import uniform, normal  # noqa: E402
import mp_kernels as mpk  # noqa: E402

mp.mp.dps = 50
JIT = mp.mpf("1e-8")


def chol(kind, x, h, logNoise):
    n, D = len(x), len(x[0])
    par = mpk.unpack(kind, h, D)
    c = mp.e ** (2 * logNoise) + JIT
    L = []
    for i in range(n):
        row = []
        for j in range(i):
            row.append((mpk.value(kind, x[i], x[j], *par) - mp.fdot(row[:j], L[j][:j])) / L[j][j])
        row.append(mp.sqrt(mpk.value(kind, x[i], x[i], *par) + c - mp.fdot(row, row)))
        L.append(row)
    return L


def linv_columns(L):
    """Column j of L^-1 (rows j .. n-1) for every j."""
    n = len(L)
    cols = []
    for j in range(n):
        xj = [1 / L[j][j]]
        for i in range(j + 1, n):
            xj.append(-mp.fdot(L[i][j:i], xj) / L[i][i])
        cols.append(xj)
    return cols


def lpd_of(kind, x, yc, h, logNoise):
    L = chol(kind, x, h, logNoise)
    n = len(L)
    z = []
    for i in range(n):
        z.append((yc[i] - mp.fdot(L[i][:i], z)) / L[i][i])
    tot = mp.mpf(0)
    log2pi = mp.log(2 * mp.pi)
    for j, xj in enumerate(linv_columns(L)):
        d = mp.fdot(xj, xj)
        a = mp.fdot(xj, z[j:])
        tot += -(log2pi - mp.log(d) + a * a / d) / 2
    return tot


def literal_513(kind, x, yc, h, logNoise):
    """(gradient over [logl..., logs, logNoise], lpd) from G = K_y^-1, eq. 5.13 as printed."""
    n, D = len(x), len(x[0])
    par = mpk.unpack(kind, h, D)
    L = chol(kind, x, h, logNoise)
    cols = linv_columns(L)
    # G = L^-T L^-1: G[i][j] = sum_k Linv[k][i] Linv[k][j], k >= max(i, j); column i of L^-1 holds rows i ..
    G = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            G[i][j] = G[j][i] = mp.fdot(cols[i], cols[j][i - j:])
    alpha = [mp.fdot(G[i], yc) for i in range(n)]
    d = [G[i][i] for i in range(n)]
    log2pi = mp.log(2 * mp.pi)
    lpd = mp.fsum(-(log2pi - mp.log(d[i]) + alpha[i] ** 2 / d[i]) / 2 for i in range(n))
    nh = len(h)
    dk = [[mpk.d_hyper(kind, x[i], x[j], *par)[1] for j in range(n)] for i in range(n)]
    grad = []
    noise2 = 2 * mp.e ** (2 * logNoise)
    for p in range(nh + 1):
        if p < nh:
            dK = [[dk[i][j][p] for j in range(n)] for i in range(n)]
        else:
            dK = [[noise2 if i == j else mp.mpf(0) for j in range(n)] for i in range(n)]
        dKc = [[dK[i][j] for i in range(n)] for j in range(n)]       # columns
        tot = mp.mpf(0)
        for i in range(n):
            Zi = [mp.fdot(G[i], dKc[j]) for j in range(n)]              # row i of Z = G dK
            za = mp.fdot(Zi, alpha)
            zg = mp.fdot(Zi, G[i])                                      # [Z G]_ii (G symmetric)
            tot += (alpha[i] * za - (1 + alpha[i] ** 2 / d[i]) * zg / 2) / d[i]
        grad.append(tot)
    return grad, lpd


# name, kind, n, D, loghyp (without the noise), logNoise, target scale, mean offset from mean(y), weak
CASES = [
    ("isose_n1_d1", 0, 1, 1, [np.log(0.2), 0.0], np.log(0.1), 1.0, 0.3, 0),
    ("ardse_n2_d8", 1, 2, 8, list(np.log(np.linspace(0.4, 0.9, 8))) + [-0.2], np.log(0.1), 1.0, 0.0, 0),
    ("isolinear_n127_d8", 2, 127, 8, [np.log(1.5), 0.0], np.log(0.1), 1.0, 0.0, 0),
    ("ardlinear_n129_d8", 3, 129, 8, list(np.log(np.linspace(0.8, 1.6, 8))) + [0.0], np.log(0.1), 1.0, 0.7, 0),
    ("ardseproduct_n128_d8", 4, 128, 8, list(np.log(np.linspace(0.6, 1.4, 8))) + [-0.1], np.log(0.1), 1.0, 0.0, 0),
    ("isomatern32_n300_d1", 5, 300, 1, [np.log(0.3), 0.0], np.log(0.1), 1.0, 0.0, 0),
    ("isomatern52_n64_d40", 6, 64, 40, [np.log(3.0), 0.1], np.log(0.1), 1.0, -0.4, 0),
    ("ardmatern32_n129_d8", 7, 129, 8, list(np.log(np.linspace(0.8, 1.8, 8))) + [0.0], np.log(0.1), 1.0, 0.0, 0),
    ("ardmatern52_n48_d40", 8, 48, 40, list(np.log(np.linspace(1.5, 3.0, 40))) + [-0.1], np.log(0.1), 1.0, 0.0, 0),
    ("ardse_n64_d35", 1, 64, 35, list(np.log(np.linspace(0.5, 1.5, 35))) + [-0.5 * np.log(35.0)], np.log(0.1), 1.0, 0.0, 0),
    ("isose_n128_d1_bigy", 0, 128, 1, [np.log(0.2), np.log(30.0)], np.log(3.0), 1e3, 0.0, 0),
    ("isose_n127_d8_weak", 0, 127, 8, [np.log(0.8), 0.5 * np.log(1e-8 * (0.01 + 1e-8))], np.log(0.1), 1.0, 0.0, 1),
    ("isolinear_n128_d1_weak", 2, 128, 1, [0.5 * np.log(1.0 / (1e-8 * (0.01 + 1e-8))), 0.0], np.log(0.1), 1.0, 0.0, 1),
]


def run_case(args):
    si, (name, kind, n, D, loghyp, logNoise, yscale, moff, weak) = args
    mp.mp.dps = 50
    X = uniform(4000 + si, 0, n * D).reshape((n, D), order="F")
    y = yscale * (np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * normal(4050 + si, 0, n)) + 0.5 * yscale
    mean = float(np.mean(y)) + float(moff)
    loghyp = np.array(loghyp, dtype=np.float64)
    logNoise = float(logNoise)
    x = [[mp.mpf(float(v)) for v in r] for r in X]
    yc = [mp.mpf(float(v)) - mp.mpf(mean) for v in y]
    h = [mp.mpf(float(v)) for v in loghyp]
    ln = mp.mpf(logNoise)
    g_mp, lpd_mp = literal_513(kind, x, yc, h, ln)
    # central differences of lpd at 50 digits
    step = mp.mpf("1e-15")
    worst = mp.mpf(0)
    for p in range(len(h) + 1):
        if p == len(h) - 1 and kind in (2, 3):
            assert g_mp[p] == 0
            continue
        hp, hm, lp, lm = list(h), list(h), ln, ln
        if p < len(h):
            hp[p] += step
            hm[p] -= step
        else:
            lp, lm = ln + step, ln - step
        fd = (lpd_of(kind, x, yc, hp, lp) - lpd_of(kind, x, yc, hm, lm)) / (2 * step)
        dev = abs(fd - g_mp[p]) / max(1, abs(g_mp[p]))
        worst = max(worst, dev)
        assert dev <= mp.mpf("1e-24"), (name, p, fd, g_mp[p])
    grad = np.array([float(v) for v in g_mp])
    noise = float(np.exp(2.0 * logNoise))
    K = dense_kernels.value(kind, loghyp, X, X)
    ev = np.linalg.eigvalsh(K + (noise + lgd.JITTER) * np.eye(n))
    cond = float(f"{ev[-1] / ev[0]:.4g}")
    assert cond <= 1e6, (name, cond)
    case = dict(kind=kind, cond=cond, weak=bool(weak), logNoise=logNoise, y=y, mean=mean)
    dense = lgd.loo_grad_dense(K, dense_kernels.d_hyper(kind, loghyp, X)[1], noise, y, mean)
    ratio = float(np.max(np.abs(dense - grad) / lgd.tolerance(case, grad, K)))
    line = (f"{name:24s} kind {kind} n {n:3d} D {D:2d}  cond {cond:9.4g}  max|y| {np.max(np.abs(y)):8.3g}  |g|inf {np.max(np.abs(grad)):9.3g}  "
            f"fd dev {float(worst):.1e}  dense err / tol {ratio:.2g}")
    print(line, flush=True)
    rec = dict(X=X, y=y, loghyp=loghyp, grad=grad,
               meta=np.array([kind, mean, logNoise, cond, float(lpd_mp), weak], dtype=np.float64))
    return name, rec, ratio


def main():
    with Pool(min(len(CASES), os.cpu_count() or 1)) as pool:
        res = pool.map(run_case, list(enumerate(CASES)), chunksize=1)
    flat = {}
    for name, rec, ratio in res:
        assert ratio <= 0.05, (name, ratio)
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
    out = os.path.join(HERE, "gp_loo_grad.npz")
    mpk.savez_reproducible(out, flat, compresslevel=9)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
