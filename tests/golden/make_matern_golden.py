"""Generate tests/golden/gp_matern.npz: 50-digit references for single GP leaves with the Matern kernels (kinds 5-8).

r^2 = sum_d (a_d - b_d)^2 / l_d^2 (one l for the iso kinds), s = sqrt(2 nu) r, k(a, b) = sigma^2 (1 + s) e^-s (nu = 3/2) or
sigma^2 (1 + s + s^2 / 3) e^-s (nu = 5/2) (include/dsmgp_hip.h, DSMGP_KIND_*_MATERN*).  Every case is evaluated in mpmath at
50 digits straight from the textbook equations: K, K_y = K + (noise + 1e-8) I, its Cholesky factor L, alpha = K_y^-1 (y - mean),
K_y^-1 = L^-T L^-1, the log-marginal, the predictive moments mean + k*^T alpha and sigma^2 - |L^-1 k*|^2 + noise at a few test
points, and every gradient component as the direct contraction 0.5 tr((alpha alpha^T - K_y^-1) dK/dtheta) in the library's
order (iso [dl, ds, dnoise], ARD [dl_1..dl_D, ds, dnoise]) -- true derivatives, no factor sigma:

  dK/dlog l_d = sigma^2 e^-s c(s) s_d^2,  s_d^2 = 2 nu (a_d - b_d)^2 / l_d^2,  c = 1 (nu = 3/2), (1 + s) / 3 (nu = 5/2);
  an iso dl is the sum over d;  dK/dlog sigma = 2 K;  dK_y/dlog sigma_n = 2 noise I.

Stored with each case: the kind, the inputs, a corner of K (up to 8 x 8) and the first rows of K(X, X*), cond_2(K_y) (4 digits:
tolerance metadata).  The n = 1 and n = 2 cases must agree with their closed forms -- the n = 2 gradients are mpmath's own
numerical derivatives of the closed-form log-marginal, independent of the formula above -- before anything is written.  Cases
include duplicate training points (s = 0 off the diagonal) and length-scales spread over two decades.  The largest leaf has 300
rows: 50-digit Cholesky factors above 1,300 rows would take hours, so tests/test_matern_gpu.py checks those sizes against the dense
restatement (tests/dense_gp.py), which tests/test_matern_host.py pins to these references.  Imports numpy and mpmath only
(the data come from numpy's PCG64 generator).  Run from the repo root:
    python tests/golden/make_matern_golden.py        (a few minutes; the output is byte-reproducible)
"""
import os

import mpmath as mp
import numpy as np

from mp_kernels import d_hyper, iso_logl as _iso, savez_reproducible, spread_logl as _logl, unpack, value

OUT = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
ISO32, ISO52, ARD32, ARD52 = 5, 6, 7, 8


def _nu2(kind):
    return 3 if kind in (ISO32, ARD32) else 5


def _ard(kind):
    return kind in (ARD32, ARD52)


def _kfun(kind, logl, logs, D):
    """k(a, b) and dk/dlog l (one entry for an iso kind, D for an ARD kind) at 50 digits."""
    par = unpack(kind, [mp.mpf(float(v)) for v in logl] + [mp.mpf(float(logs))], D)
    return (lambda a, b: value(kind, a, b, *par)), (lambda a, b: d_hyper(kind, a, b, *par)[1][:-1]), par[2]


def mp_case(kind, X, y, mean, logl, logs, logNoise, Xt):
    n, D = X.shape
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    xt = [[mp.mpf(float(v)) for v in row] for row in Xt]
    k, dk, s2 = _kfun(kind, logl, logs, D)
    noise = mp.e ** (2 * mp.mpf(float(logNoise)))
    c = noise + mp.mpf("1e-8")
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
    gl = [mp.mpf(0)] * (D if _ard(kind) else 1)
    gs = mp.mpf(0)
    trW = mp.mpf(0)
    for i in range(n):
        for j in range(i + 1):
            w = alpha[i] * alpha[j] - Kinv[i][j]
            f = 1 if i == j else 2
            gs += f * w * K[i][j]
            if i == j:
                trW += w
                continue
            dki = dk(x[i], x[j])
            for d in range(len(gl)):
                gl[d] += f * w * dki[d]
    gl = [v / 2 for v in gl]
    grad = gl + [gs, noise * trW]
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


def closed_form(kind, X, y, mean, logl, logs, logNoise):
    """n = 1 and n = 2 written out by hand: [grad..., mll].  For n = 2 the gradients are mp.diff of the closed-form mll."""
    n, D = X.shape
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    yc = [mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y]
    nl = D if _ard(kind) else 1
    if n == 1:         # K = sigma^2: no length-scale term, ds = p sigma^2
        s2 = mp.e ** (2 * mp.mpf(float(logs)))
        noise = mp.e ** (2 * mp.mpf(float(logNoise)))
        c = noise + mp.mpf("1e-8")
        a = yc[0] / (s2 + c)
        p = a * a - 1 / (s2 + c)
        mll = -(yc[0] * a + mp.log(s2 + c) + mp.log(2 * mp.pi)) / 2
        return [mp.mpf(0)] * nl + [p * s2, noise * p, mll]
    nu2 = _nu2(kind)

    def f(*th):        # th = [logl..., logs, logNoise]
        ll = th[:nl]
        r2 = sum((x[0][d] - x[1][d]) ** 2 / mp.e ** (2 * ll[d if _ard(kind) else 0]) for d in range(D))
        s = mp.sqrt(nu2 * r2)
        s2 = mp.e ** (2 * th[nl])
        b = s2 * (1 + s + (s * s / 3 if nu2 == 5 else 0)) * mp.e ** (-s)
        a = s2 + mp.e ** (2 * th[nl + 1]) + mp.mpf("1e-8")
        det = a * a - b * b
        quad = (a * yc[0] ** 2 - 2 * b * yc[0] * yc[1] + a * yc[1] ** 2) / det
        return -(quad + mp.log(det) + 2 * mp.log(2 * mp.pi)) / 2

    th = [mp.mpf(float(v)) for v in logl][:nl] + [mp.mpf(float(logs)), mp.mpf(float(logNoise))]
    grads = []
    for j in range(len(th)):
        def fj(t, j=j):
            u = list(th)
            u[j] = t
            return f(*u)
        grads.append(mp.diff(fj, th[j]))
    return grads + [f(*th)]


# name, kind, n, D, logl, logs, logNoise, target offset (the leaf's mean stays 0: the kernel carries it), duplicated rows
SPECS = [
    ("n1_iso32_d3", ISO32, 1, 3, _iso(3), 0.1, np.log(0.2), 0.0, 0),
    ("n1_ard52_d3", ARD52, 1, 3, _logl(3), 0.1, np.log(0.2), 0.0, 0),
    ("n2_iso32_d3", ISO32, 2, 3, _iso(3), -0.2, np.log(0.2), 0.0, 0),
    ("n2_iso52_d2", ISO52, 2, 2, _iso(2), 0.3, np.log(0.2), 0.0, 0),
    ("n2_ard32_d3", ARD32, 2, 3, _logl(3), -0.2, np.log(0.2), 0.0, 0),
    ("n2_ard52_d4", ARD52, 2, 4, _logl(4), 0.1, np.log(0.3), 0.0, 0),
    ("n127_iso32_d1", ISO32, 127, 1, _iso(1), 0.0, np.log(0.2), 0.0, 0),
    ("n127_ard52_d1", ARD52, 127, 1, _logl(1), 0.0, np.log(0.2), 0.0, 0),
    ("n128_iso52_d3", ISO52, 128, 3, _iso(3), 0.2, np.log(0.2), 0.0, 0),
    ("n128_ard32_d3", ARD32, 128, 3, _logl(3), 0.2, np.log(0.2), 0.0, 0),
    ("n129_ard52_d8", ARD52, 129, 8, _logl(8), 0.0, np.log(0.2), 0.0, 0),
    ("n129_iso32_d8", ISO32, 129, 8, _iso(8), 0.0, np.log(0.2), 0.0, 0),
    ("n300_ard52_d8", ARD52, 300, 8, _logl(8), -0.1, np.log(0.25), 0.0, 0),
    ("n129_ard52_d48", ARD52, 129, 48, _logl(48), 0.0, np.log(0.2), 0.0, 0),
    ("spread_ard52_d8", ARD52, 129, 8, np.log(np.geomspace(0.05, 5.0, 8)), 0.0, np.log(0.2), 0.0, 0),
    ("spread_ard32_d8", ARD32, 129, 8, np.log(np.geomspace(0.05, 5.0, 8)), 0.0, np.log(0.2), 0.0, 0),
    ("dup_iso52_d3", ISO52, 140, 3, _iso(3), 0.0, np.log(0.3), 0.0, 24),
    ("dup_ard32_d3", ARD32, 140, 3, _logl(3), 0.0, np.log(0.3), 0.0, 24),
    ("offset_iso32_d3", ISO32, 128, 3, _iso(3), 0.5, np.log(0.2), 3.0, 0),
]


def main():
    flat = {}
    for si, (name, kind, n, D, logl, logs, logNoise, offset, dup) in enumerate(SPECS):
        rng = np.random.Generator(np.random.PCG64(5000 + si))
        X = rng.random((n, D))
        if dup:            # the last `dup` rows repeat earlier ones: s = 0 off the diagonal
            X[n - dup:] = X[rng.choice(n - dup, dup, replace=False)]
        y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n) + offset
        Xt = rng.random((6, D))
        mean = 0.0 if (n <= 2 or offset != 0.0) else float(np.mean(y))
        r = mp_case(kind, X, y, mean, logl, logs, logNoise, Xt)
        if n <= 2:
            cf = closed_form(kind, X, y, mean, logl, logs, logNoise)
            for a, b in zip(r["grad"] + [r["mll"]], cf):
                assert abs(a - b) <= mp.mpf("1e-30") * max(1, abs(b)), (name, a, b)
        ev = np.linalg.eigvalsh(r["Ky"])
        cond = float(f"{ev[-1] / ev[0]:.4g}")
        rec = dict(kind=kind, X=X, y=y, Xt=Xt, mean=mean, logl=np.asarray(logl, dtype=np.float64), logs=float(logs),
                   logNoise=float(logNoise), grad=np.array([float(v) for v in r["grad"]]), mll=float(r["mll"]),
                   mu=np.array([float(v) for v in r["mu"]]), var=np.array([float(v) for v in r["var"]]),
                   Kc=r["Kc"], Kt=r["Kt"], cond=cond)
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
        print(f"{name:16s} kind {kind} n {n:3d} D {D:2d}  cond {cond:9.4g}  mll {float(r['mll']):12.6g}  "
              f"|g|inf {np.max(np.abs(rec['grad'])):9.3g}", flush=True)
    savez_reproducible(os.path.join(OUT, "gp_matern.npz"), flat)


if __name__ == "__main__":
    main()
