"""Generate tests/golden/gp_kfold.npz: 50-digit k-fold moments of single leaves, from the definition.

For every label k the GP is refitted in mpmath at 50 digits without the rows of the fold -- same mean, same hyper-parameters,
K_y = K + (noise + 1e-8) I -- and predicts the fold's rows jointly: mu = m + K_Fr K_y,rr^-1 (y_r - m), Sigma = K_y,FF - K_Fr
K_y,rr^-1 K_rF, lpd = log N(y_F | mu, Sigma).  Stored per case: the inputs, the labels, mu and var = diag Sigma per row (NaN for
label -1), lpd per label, kss, lpd_abs (the sum of the absolute terms of the density: quadratic half, |log| of every pivot of
chol(Sigma), (m / 2) log 2 pi) and lpd_err: the error of the float64 dense helper (tests/kfold_dense.py, the single-fit formulas)
against the 50-digit value, per block; the case's error, the largest of them, goes into `meta`, and the device tolerance of lpd
is taken from that one (the blocks of a case share K_y and its condition: a single block's error is one sample of it).

Cases: the inputs of gp_loo.npz with n <= 140 (IsoSE n = 127, ArdSE n = 128, ArdLinear n = 129, ArdMatern52 n = 129, D = 40) and
an IsoRQ leaf of this file's own (n = 96, D = 3); each with K = 3 random labels and with a second labelling that contains -1.
Asserted before anything is stored: the dense helper stays within 1/20 of the moments' tolerances on every case.
Run from the repo root:  python tests/golden/make_kfold_golden.py   (a few minutes; the output is byte-reproducible)
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
import kfold_dense  # noqa: E402
import loo_dense  # noqa: E402
import mp_kernels as mk  # noqa: E402
from make_pred_golden import uniform, normal  # noqa: E402

mp.mp.dps = 50
JIT = mp.mpf("1e-8")


def mp_chol(A):
    """Lower Cholesky factor of a symmetric matrix given by its lower triangle (lists of mpf)."""
    L = []
    for i in range(len(A)):
        row = []
        for j in range(i):
            row.append((A[i][j] - mp.fdot(row[:j], L[j][:j])) / L[j][j])
        row.append(mp.sqrt(A[i][i] - mp.fdot(row, row)))
        L.append(row)
    return L


def mp_fwd(L, b):
    z = []
    for i in range(len(L)):
        z.append((b[i] - mp.fdot(L[i][:i], z)) / L[i][i])
    return z


def mp_kfold(Ky, y, mean, labels, K):
    """(mu, var per row -- None for label -1 --, lpd, lpd_abs per label) from K_y (full symmetric lists of mpf)."""
    n = len(y)
    m0 = mp.mpf(float(mean))
    yc = [mp.mpf(float(v)) - m0 for v in y]
    mu, var, lpd, lab = [None] * n, [None] * n, [], []
    log2pi = mp.log(2 * mp.pi)
    for k in range(K):
        F = [i for i in range(n) if labels[i] == k]
        R = [i for i in range(n) if labels[i] != k]
        if not F:
            lpd.append(mp.mpf(0))
            lab.append(mp.mpf(0))
            continue
        L = mp_chol([[Ky[i][j] for j in R[:a + 1]] for a, i in enumerate(R)])
        zr = mp_fwd(L, [yc[i] for i in R])
        V = [mp_fwd(L, [Ky[i][f] for i in R]) for f in F]            # L^-1 K_rF, column by column
        m = [m0 + mp.fdot(V[a], zr) for a in range(len(F))]
        S = [[Ky[F[a]][F[b]] - mp.fdot(V[a], V[b]) for b in range(a + 1)] for a in range(len(F))]
        C = mp_chol(S)
        r = mp_fwd(C, [mp.mpf(float(y[f])) - m[a] for a, f in enumerate(F)])
        q = mp.fdot(r, r) / 2
        logs = [mp.log(C[a][a]) for a in range(len(F))]
        lpd.append(-q - mp.fsum(logs) - len(F) * log2pi / 2)
        lab.append(q + mp.fsum(abs(v) for v in logs) + len(F) * log2pi / 2)
        for a, f in enumerate(F):
            mu[f], var[f] = m[a], S[a][a]
    return mu, var, lpd, lab


def labellings(n, seed):
    """K = 3 random labels, and a labelling over -1 .. 2 (about a quarter of the rows never held out)."""
    a = np.minimum((uniform(seed, 0, n) * 3).astype(np.int32), 2)
    b = np.minimum((uniform(seed + 1, 0, n) * 4).astype(np.int32), 3) - 1
    return {"k3": a.astype(np.int32), "k3_unheld": b.astype(np.int32)}


def main():
    loo = loo_dense.load_cases()
    inputs = []
    for name in ("isose_n127", "ardse_n128", "ardlinear_n129", "ardmatern52_n129_d40"):
        c = loo[name]
        inputs.append((name, c["kind"], c["X"], c["y"], c["loghyp"], c["logNoise"], c["mean"]))
    n, D = 96, 3
    X = uniform(3300, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * normal(3301, 0, n) + 0.5
    inputs.append(("isorq_n96", 9, X, y, np.array([np.log(0.6), np.log(1.5), -0.1]), np.log(0.1), float(np.mean(y))))
    K = 3
    flat = {}
    for si, (name, kind, X, y, loghyp, logNoise, mean) in enumerate(inputs):
        n, D = X.shape
        h = [mp.mpf(float(v)) for v in loghyp]
        il2, al, s2 = mk.unpack(kind, h, D)
        xs = [[mp.mpf(float(v)) for v in r] for r in X]
        noise = mp.e ** (2 * mp.mpf(float(logNoise)))
        low = [[mk.value(kind, xs[i], xs[j], il2, al, s2) for j in range(i + 1)] for i in range(n)]
        Ky = [[low[max(i, j)][min(i, j)] + (noise + JIT if i == j else 0) for j in range(n)] for i in range(n)]
        kss = np.array([float(low[i][i]) for i in range(n)])
        ev = np.linalg.eigvalsh(np.array([[float(v) for v in row] for row in Ky]))
        cond = float(f"{ev[-1] / ev[0]:.4g}")
        assert cond <= 1e6, (name, cond)
        Kd = dk.value(kind, loghyp, X, X)
        for tag, labels in labellings(n, 3400 + 10 * si).items():
            mu_mp, var_mp, lpd_mp, lab_mp = mp_kfold(Ky, y, mean, labels, K)
            mu = np.array([np.nan if v is None else float(v) for v in mu_mp])
            var = np.array([np.nan if v is None else float(v) for v in var_mp])
            dm, dv, dl = kfold_dense.kfold_dense(Kd, float(noise), y, mean, labels, K)
            lpd_err = np.array([abs(float(mp.mpf(float(d)) - v)) for d, v in zip(dl, lpd_mp)])
            held = labels >= 0
            tm, tv = kfold_dense.moment_tols(y, mu, var, kss, float(noise))
            ratios = [float(np.max(np.abs(dm - mu)[held] / tm[held])), float(np.max(np.abs(dv - var)[held] / tv[held]))]
            assert max(ratios) <= 0.05, (name, tag, ratios)
            assert np.array_equal(np.isnan(dm), ~held)
            rec = dict(X=X, y=y, loghyp=np.asarray(loghyp, dtype=np.float64), labels=labels.astype(np.int32), mu=mu, var=var,
                       lpd=np.array([float(v) for v in lpd_mp]), lpd_abs=np.array([float(v) for v in lab_mp]), lpd_err=lpd_err,
                       kss=kss, meta=np.array([kind, mean, logNoise, cond, K, float(np.max(lpd_err))], dtype=np.float64))
            for k, v in rec.items():
                flat[f"{name}_{tag}/{k}"] = np.asarray(v)
            print(f"{name + '_' + tag:34s} kind {kind} n {n:3d} cond {cond:9.4g} sizes {[int(np.sum(labels == k)) for k in range(K)]} "
                  f"dense err / tol: mu {ratios[0]:.2g} var {ratios[1]:.2g}; lpd err {np.array2string(lpd_err, precision=2)} "
                  f"floor {np.array2string(kfold_dense.lpd_floor([np.sum(labels == k) for k in range(K)], rec['lpd_abs']), precision=2)}",
                  flush=True)
    out = os.path.join(HERE, "gp_kfold.npz")
    mk.savez_reproducible(out, flat)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
