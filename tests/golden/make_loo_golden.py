"""Generate tests/golden/gp_loo.npz: 50-digit leave-one-out moments of single leaves.

Leave-one-out cross-validation of an exact GP (GPML 5.4.2, eqs. 5.10-5.12) with the mean and the hyper-parameters held fixed:
d_i = [K_y^-1]_ii, alpha = K_y^-1 (y - m), mu_i = y_i - alpha_i / d_i, var_i = 1 / d_i,
lpd_i = -(log 2pi + log var_i + (y_i - mu_i)^2 / var_i) / 2.  Everything is evaluated in mpmath at 50 digits from the float64
inputs the device reads: the kernel matrix, K_y = K + (noise + 1e-8) I, its Cholesky factor (MPCov of make_predcov_golden.py),
L^-1 column by column, alpha = L^-T (L^-1 (y - m)).

Cases: n in {1, 127, 128, 129, 300} (one tile short by a row, a full tile, one row into the second tile, three tiles -- the
device adds its row sums in slices of 256 columns); D in {1, 8, 40}; IsoSE, ArdSE, ArdLinear, ArdMatern52; every mean is
non-zero, one differs from mean(y); one case has targets of magnitude 1e3.

Conditions on the inputs, asserted before anything is stored: cond_2(K_y) <= 1e6, and the float64 dense helper
(tests/loo_dense.py) stays within 1/100 of the tolerances of loo_dense.loo_tol on every case.
Run from the repo root:  python tests/golden/make_loo_golden.py   (a few minutes; the output is byte-reproducible)
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import dense_kernels as dk  # noqa: E402
import loo_dense  # noqa: E402
from make_pred_golden import uniform, normal  # noqa: E402
from make_predcov_golden import MPCov, savez_reproducible  # noqa: E402

mp.mp.dps = 50


def mp_loo(g, y, mean):
    """(mu, var, lpd_i, kss) of the leaf `g` (an MPCov: its 50-digit factor) as lists of mpf."""
    n = len(g.x)
    L = g.L
    yc = [mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y]
    z = []
    for i in range(n):
        z.append((yc[i] - mp.fdot(L[i][:i], z)) / L[i][i])
    mu, var, lpd = [], [], []
    log2pi = mp.log(2 * mp.pi)
    for j in range(n):
        x = [1 / L[j][j]]                       # column j of L^-1, rows j .. n-1
        for i in range(j + 1, n):
            x.append(-mp.fdot(L[i][j:i], x) / L[i][i])
        d = mp.fdot(x, x)
        a = mp.fdot(x, z[j:])
        yj = mp.mpf(float(y[j]))
        m, v = yj - a / d, 1 / d
        mu.append(m)
        var.append(v)
        lpd.append(-(log2pi + mp.log(v) + (yj - m) ** 2 / v) / 2)
    kss = [g.k(xi, xi) for xi in g.x]
    return mu, var, lpd, kss


# name, kind, n, D, loghyp (library hyper-vector without the noise), logNoise, target scale, mean (None: mean(y))
CASES = [
    ("isose_n1", 0, 1, 1, [np.log(0.2), 0.0], np.log(0.1), 1.0, 0.3),
    ("isose_n127", 0, 127, 1, [np.log(0.2), 0.0], np.log(0.1), 1.0, None),
    ("ardse_n128", 1, 128, 8, list(np.log(np.linspace(0.4, 0.9, 8))) + [-0.2], np.log(0.1), 1.0, None),
    ("ardlinear_n129", 3, 129, 8, list(np.log(np.linspace(0.5, 1.2, 8))) + [0.0], np.log(0.1), 1.0, 0.7),
    ("ardmatern52_n129_d40", 8, 129, 40, list(np.log(np.linspace(1.5, 3.0, 40))) + [-0.1], np.log(0.1), 1.0, None),
    ("isose_n300_bigy", 0, 300, 1, [np.log(0.2), np.log(30.0)], np.log(3.0), 1e3, None),
]


def main():
    flat = {}
    for si, (name, kind, n, D, loghyp, logNoise, yscale, mean) in enumerate(CASES):
        X = uniform(3000 + si, 0, n * D).reshape((n, D), order="F")
        y = yscale * (np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * normal(3050 + si, 0, n)) + 0.5 * yscale
        mean = float(np.mean(y)) if mean is None else float(mean)
        loghyp = np.array(loghyp, dtype=np.float64)
        g = MPCov(kind, loghyp, logNoise, X)
        assert g.cond <= 1e6, (name, g.cond)
        mu_mp, var_mp, lpd_mp, kss_mp = mp_loo(g, y, mean)
        mu, var, lpd, kss = (np.array([float(v) for v in a]) for a in (mu_mp, var_mp, lpd_mp, kss_mp))
        lpd_sum = float(mp.fsum(lpd_mp))
        noise = float(g.noise)
        # the float64 helper against 50 digits: within 1/100 of the tolerances
        dm, dv, dl = loo_dense.loo_dense(dk.value(kind, loghyp, X, X), noise, y, mean)
        tm, tv, tl, ts = loo_dense.loo_tol(y, mu, var, kss, noise)
        ratios = [float(np.max(np.abs(dm - mu) / tm)), float(np.max(np.abs(dv - var) / tv)), float(np.max(np.abs(dl - lpd) / tl)),
                  abs(float(np.sum(dl)) - lpd_sum) / ts]
        assert max(ratios) <= 0.01, (name, ratios)
        rec = dict(X=X, y=y, loghyp=loghyp, mu=mu, var=var, lpd=lpd, kss=kss,
                   meta=np.array([kind, mean, logNoise, g.cond, lpd_sum], dtype=np.float64))
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
        print(f"{name:22s} kind {kind} n {n:3d} D {D:2d}  cond {g.cond:9.4g}  max|y| {np.max(np.abs(y)):8.3g}  "
              f"dense err / tol: mu {ratios[0]:.2g} var {ratios[1]:.2g} lpd {ratios[2]:.2g} sum {ratios[3]:.2g}", flush=True)
    out = os.path.join(HERE, "gp_loo.npz")
    savez_reproducible(out, flat)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
