"""Generate tests/golden/gp_ardse_product.npz: 50-digit references for single GP leaves with the ArdSEProduct kernel.

k(a, b) = sigma^2 exp(-0.5 sum_d (a_d - b_d)^2 / l_d^2) (include/dsmgp_hip.h, DSMGP_KIND_ARD_SE_PRODUCT).  Every case is
evaluated in mpmath at 50 digits straight from the textbook equations: K, K_y = K + (noise + 1e-8) I, its Cholesky factor L,
alpha = K_y^-1 (y - mean), K_y^-1 = L^-T L^-1, the log-marginal, the predictive moments mean + k*^T alpha and
sigma^2 - |L^-1 k*|^2 + noise at a few test points, and every gradient component as the direct contraction
0.5 tr((alpha alpha^T - K_y^-1) dK/dtheta) in the library's order [dl_1..dl_D, ds, dnoise] -- true derivatives, no factor sigma:

  dK/dlog l_d = K o (a_d - b_d)^2 / l_d^2,   dK/dlog sigma = 2 K,   dK_y/dlog sigma_n = 2 noise I.

Stored with each case: the inputs, a corner of K (up to 8 x 8) and the first rows of K(X, X*), cond_2(K_y) (4 digits:
tolerance metadata).  The n = 1 and n = 2 cases must agree with their closed forms before anything is written.  Imports numpy and
mpmath only (the data come from numpy's PCG64 generator).  Run from the repo root:
    python tests/golden/make_ardse_product_golden.py        (a minute or two; the output is byte-reproducible)
"""
import os

import mpmath as mp
import numpy as np

from mp_kernels import savez_reproducible, spread_logl as _logl, value

OUT = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50


def mp_case(X, y, mean, logl, logs, logNoise, Xt):
    n, D = X.shape
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    xt = [[mp.mpf(float(v)) for v in row] for row in Xt]
    il2 = [1 / mp.e ** (2 * mp.mpf(float(v))) for v in logl]
    s2 = mp.e ** (2 * mp.mpf(float(logs)))
    noise = mp.e ** (2 * mp.mpf(float(logNoise)))
    c = noise + mp.mpf("1e-8")

    def k(a, b):
        return value(4, a, b, il2, None, s2)

    K = [[k(x[i], x[j]) for j in range(i + 1)] for i in range(n)]
    full = lambda A, i, j: A[i][j] if j <= i else A[j][i]      # noqa: E731
    Ky = [[K[i][j] + (c if i == j else 0) for j in range(i + 1)] for i in range(n)]
    L = []
    for i in range(n):
        row = []
        for j in range(i):
            row.append((Ky[i][j] - mp.fdot(row[:j], L[j][:j])) / L[j][j])
        row.append(mp.sqrt(Ky[i][i] - mp.fdot(row, row)))
        L.append(row)
    col = []                                                    # columns of L^-1: col[j][k - j] = (L^-1)[k][j]
    for j in range(n):
        cj = [1 / L[j][j]]
        for i in range(j + 1, n):
            cj.append(-mp.fdot(L[i][j:i], cj) / L[i][i])
        col.append(cj)
    Kinv = [[mp.fdot(col[i], col[j][i - j:]) for j in range(i + 1)] for i in range(n)]
    yc = [mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y]
    alpha = [mp.fdot([full(Kinv, i, j) for j in range(n)], yc) for i in range(n)]
    mll = -(mp.fdot(yc, alpha) + 2 * sum(mp.log(L[i][i]) for i in range(n)) + n * mp.log(2 * mp.pi)) / 2
    # gradients: W = alpha alpha^T - K_y^-1 contracted entry by entry (off-diagonal entries twice)
    gl = [mp.mpf(0)] * D
    gs = mp.mpf(0)
    trW = mp.mpf(0)
    for i in range(n):
        for j in range(i + 1):
            w = alpha[i] * alpha[j] - Kinv[i][j]
            wk = (1 if i == j else 2) * w * K[i][j]
            gs += wk
            if i == j:
                trW += w
                continue
            for d in range(D):
                gl[d] += wk * (x[i][d] - x[j][d]) ** 2 * il2[d]
    grad = [v / 2 for v in gl] + [gs, noise * trW]
    # predictive moments
    mu, var = [], []
    for t in range(len(xt)):
        ks = [k(x[i], xt[t]) for i in range(n)]
        v = []
        for i in range(n):
            v.append((ks[i] - mp.fdot(L[i][:i], v)) / L[i][i])
        mu.append(mp.mpf(float(mean)) + mp.fdot(ks, alpha))
        var.append(s2 - mp.fdot(v, v) + noise)
    m = min(n, 8)
    Kc = np.array([[float(full(K, i, j)) for j in range(m)] for i in range(m)])
    Kt = np.array([[float(k(x[i], xt[t])) for t in range(len(xt))] for i in range(m)])
    Kyf = np.array([[float(full(Ky, i, j)) for j in range(n)] for i in range(n)])
    return dict(grad=grad, mll=mll, mu=mu, var=var, Kc=Kc, Kt=Kt, Ky=Kyf)


def closed_form(X, y, mean, logl, logs, logNoise):
    """n = 1 and n = 2 written out by hand: [grad..., mll]."""
    n, D = X.shape
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    yc = [mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y]
    s2 = mp.e ** (2 * mp.mpf(float(logs)))
    noise = mp.e ** (2 * mp.mpf(float(logNoise)))
    c = noise + mp.mpf("1e-8")
    if n == 1:         # K = sigma^2: no length-scale term, ds = p sigma^2
        a = yc[0] / (s2 + c)
        p = a * a - 1 / (s2 + c)
        mll = -(yc[0] * a + mp.log(s2 + c) + mp.log(2 * mp.pi)) / 2
        return [mp.mpf(0)] * D + [p * s2, noise * p, mll]
    q = [(x[0][d] - x[1][d]) ** 2 / mp.e ** (2 * mp.mpf(float(logl[d]))) for d in range(D)]
    a, b = s2 + c, s2 * mp.e ** (-sum(q) / 2)
    det = a * a - b * b
    al = [(a * yc[0] - b * yc[1]) / det, (a * yc[1] - b * yc[0]) / det]
    P00, P11, P01 = al[0] ** 2 - a / det, al[1] ** 2 - a / det, al[0] * al[1] + b / det
    mll = -(yc[0] * al[0] + yc[1] * al[1] + mp.log(det) + 2 * mp.log(2 * mp.pi)) / 2
    return [P01 * b * q[d] for d in range(D)] + [(P00 + P11) * s2 + 2 * P01 * b, noise * (P00 + P11), mll]


# name, n, D, logl, logs, logNoise, target offset (the leaf's mean stays 0: the kernel carries it)
SPECS = [
    ("n1_d3", 1, 3, _logl(3), 0.1, np.log(0.2), 0.0),
    ("n2_d3", 2, 3, _logl(3), -0.2, np.log(0.2), 0.0),
    ("n127_d1", 127, 1, _logl(1), 0.0, np.log(0.2), 0.0),
    ("n128_d3", 128, 3, _logl(3), 0.2, np.log(0.2), 0.0),
    ("n129_d8", 129, 8, _logl(8), 0.0, np.log(0.2), 0.0),
    ("n257_d8", 257, 8, _logl(8), -0.1, np.log(0.25), 0.0),
    ("n160_d33", 160, 33, _logl(33), 0.0, np.log(0.2), 0.0),
    ("n160_d48", 160, 48, _logl(48), 0.0, np.log(0.2), 0.0),
    ("spread_d8", 129, 8, np.log(np.geomspace(0.05, 20.0, 8)), 0.0, np.log(0.2), 0.0),
    ("offset_d3", 128, 3, _logl(3), 0.5, np.log(0.2), 3.0),
]


def main():
    flat = {}
    for si, (name, n, D, logl, logs, logNoise, offset) in enumerate(SPECS):
        rng = np.random.Generator(np.random.PCG64(4000 + si))
        X = rng.random((n, D))
        y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n) + offset
        Xt = rng.random((6, D))
        mean = 0.0 if (n <= 2 or offset != 0.0) else float(np.mean(y))
        r = mp_case(X, y, mean, logl, logs, logNoise, Xt)
        if n <= 2:
            cf = closed_form(X, y, mean, logl, logs, logNoise)
            for a, b in zip(r["grad"] + [r["mll"]], cf):
                assert abs(a - b) <= mp.mpf("1e-40") * max(1, abs(b)), (name, a, b)
        ev = np.linalg.eigvalsh(r["Ky"])
        cond = float(f"{ev[-1] / ev[0]:.4g}")
        rec = dict(X=X, y=y, Xt=Xt, mean=mean, logl=np.asarray(logl, dtype=np.float64), logs=float(logs),
                   logNoise=float(logNoise), grad=np.array([float(v) for v in r["grad"]]), mll=float(r["mll"]),
                   mu=np.array([float(v) for v in r["mu"]]), var=np.array([float(v) for v in r["var"]]),
                   Kc=r["Kc"], Kt=r["Kt"], cond=cond)
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
        print(f"{name:10s} n {n:3d} D {D:2d}  cond {cond:9.4g}  mll {float(r['mll']):12.6g}  "
              f"|g|inf {np.max(np.abs(rec['grad'])):9.3g}", flush=True)
    savez_reproducible(os.path.join(OUT, "gp_ardse_product.npz"), flat)


if __name__ == "__main__":
    main()
