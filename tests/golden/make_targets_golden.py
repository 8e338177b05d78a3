"""Generate tests/golden/gp_targets.npz: 50-digit references for several target columns on one factorisation.

For a single leaf with inputs X, targets Y (n x Q), per-column means m and K_y = K + (noise + 1e-8) I = L L^T:
  Z = L^-1 (Y - m),   mll_j = -(|Z[:, j]|^2 + 2 sum_i log L_ii + n log 2pi) / 2,   mu[t, j] = m_j + (L^-1 k_t) . Z[:, j]
(dsmgp_solve_targets / dsmgp_predict_targets).  Everything is evaluated with mpmath at 50 digits (mpmath imported on the
machine that wrote the file: the extended-precision fall-back of the other generators was not needed) from the float64 inputs
the device reads, with the 50-digit leaf of make_predcov_golden.py (MPCov: kernel matrix, Cholesky factor, any kernel kind).

Cases (Q = 3 everywhere: a smooth column, a second function with an offset of 1000, a column of noise; a few test rows each --
one AT a training input, one 1e-7 away, the rest inside and outside the data):
  isose_n37       IsoSE, D = 2, one partial 128-block
  ardmatern52_n129  ArdMatern52, D = 3: a second block of one row
  isolinear_n130  IsoLinear, D = 2
  isose_floor_n60   IsoSE, D = 2, noise variance 1e-8 -- AT the 1e-8 jitter the fit adds, cond_2(K_y) ~ 1e9: the manner of
                  gp_edge.npz pushed to the floor
Each case stores X, Y, mean, loghyp, Z, mll, Xt, mu and meta = [kind, logNoise, cond_2(K_y)].  Before anything is stored the
float64 dense restatement (tests/targets_dense.py on SciPy's Cholesky) must agree with the 50 digits within its own tolerance.
Run from the repo root:  python tests/golden/make_targets_golden.py   (about a minute; the output is byte-reproducible)
"""
import os
import sys

import mpmath as mp
import numpy as np
import scipy.linalg as sla

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

from make_pred_golden import uniform, normal  # noqa: E402
from make_predcov_golden import MPCov, savez_reproducible  # noqa: E402
import targets_dense  # noqa: E402

mp.mp.dps = 50

# name, kind, n, D, test rows, loghyp (library hyper-vector without the noise), logNoise
CASES = [
    ("isose_n37", 0, 37, 2, 5, [np.log(0.35), 0.1], np.log(0.1)),
    ("ardmatern52_n129", 8, 129, 3, 6, list(np.log([0.5, 0.8, 0.6])) + [-0.1], np.log(0.1)),
    ("isolinear_n130", 2, 130, 2, 5, [np.log(0.9), 0.0], np.log(0.1)),
    ("isose_floor_n60", 0, 60, 2, 5, [np.log(0.15), 0.0], np.log(1e-4)),
]


def targets(si, X):
    n = X.shape[0]
    return np.stack([np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * normal(3100 + si, 0, n),
                     1000.0 + np.cos(5.0 * X[:, 0]) + X[:, -1] + 0.05 * normal(3200 + si, 0, n),
                     normal(3300 + si, 0, n)], axis=1)


def mp_targets(g, Y, mean, Xt):
    """(Z, mll, mu) at 50 digits on the factor of the MPCov leaf `g`."""
    n, Q = Y.shape
    L = g.L
    logdet = 2 * mp.fsum(mp.log(L[i][i]) for i in range(n))
    Z, mll = [], []
    for j in range(Q):
        r = [mp.mpf(float(Y[i, j])) - mp.mpf(float(mean[j])) for i in range(n)]
        z = []
        for i in range(n):
            z.append((r[i] - mp.fdot(L[i][:i], z)) / L[i][i])
        Z.append(z)
        mll.append(-(mp.fdot(z, z) + logdet + n * mp.log(2 * mp.pi)) / 2)
    mu = []
    for x in Xt:
        xs = g.row(x)
        ks = [g.k(xi, xs) for xi in g.x]
        v = []
        for i in range(n):
            v.append((ks[i] - mp.fdot(L[i][:i], v)) / L[i][i])
        mu.append([mp.mpf(float(mean[j])) + mp.fdot(v, Z[j]) for j in range(Q)])
    f = lambda a: np.array([[float(v) for v in row] for row in a])      # noqa: E731
    return f(Z).T.copy(), np.array([float(v) for v in mll]), f(mu)


def main():
    flat = {}
    for si, (name, kind, n, D, R, loghyp, logNoise) in enumerate(CASES):
        X = uniform(3000 + si, 0, n * D).reshape((n, D), order="F")
        Y = targets(si, X)
        mean = np.mean(Y, axis=0)
        Xt = uniform(3400 + si, 0, R * D).reshape((R, D), order="F") * 1.4 - 0.2
        Xt[0] = X[n - 1]
        Xt[1] = X[0] + 1e-7
        loghyp = np.array(loghyp, dtype=np.float64)
        g = MPCov(kind, loghyp, logNoise, X)
        Z, mll, mu = mp_targets(g, Y, mean, Xt)
        # the float64 restatement on SciPy's factor of the same matrix, at its own tolerances
        Ky = np.array([[float(g.k(g.x[i], g.x[j])) for j in range(n)] for i in range(n)])
        Ky[np.diag_indices(n)] += float(g.noise) + 1e-8
        F = sla.cholesky(Ky, lower=True)
        Ktn = np.array([[float(g.k(g.row(x), xi)) for xi in g.x] for x in Xt])
        cond = targets_dense.factor_cond(F)
        dZ, dmll, dmu = targets_dense.reference(F, Y, mean, Ktn)
        rz = float(np.max(np.abs(dZ - Z) / targets_dense.z_tol(Z, cond)))
        rm = float(np.max(np.abs(dmll - mll) / targets_dense.mll_tol(Z, F, cond)))
        ru = float(np.max(np.abs(dmu - mu) / targets_dense.mu_tol(mu, Y)))
        assert max(rz, rm, ru) <= 1.0, (name, rz, rm, ru)
        rec = dict(X=X, Y=Y, mean=mean, loghyp=loghyp, Z=Z, mll=mll, Xt=Xt, mu=mu,
                   meta=np.array([kind, logNoise, g.cond], dtype=np.float64))
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
        print(f"{name:18s} kind {kind} n {n:3d} D {D}  cond {g.cond:9.4g}  dense err / tol: Z {rz:.2g} mll {rm:.2g} mu {ru:.2g}",
              flush=True)
    out = os.path.join(HERE, "gp_targets.npz")
    savez_reproducible(out, flat)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
