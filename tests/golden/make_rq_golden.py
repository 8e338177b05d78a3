"""Generate tests/golden/gp_rq.npz: 50-digit references for single GP leaves with the rational quadratic kernels (kinds 9, 10).

w = sum_d (a_d - b_d)^2 / (2 alpha l_d^2) (one l for the iso kind), k(a, b) = sigma^2 (1 + w)^-alpha, alpha = exp(loga)
(include/dsmgp_hip.h, DSMGP_KIND_ISO_RQ / DSMGP_KIND_ARD_RQ).  Every case is evaluated in mpmath at 50 digits straight from the
textbook equations: K, K_y = K + (noise + 1e-8) I, its Cholesky factor L, G = K_y^-1 = L^-T L^-1, alpha = G (y - mean), and

  the log-marginal and the predictive moments mean + k*^T alpha, sigma^2 - |L^-1 k*|^2 + noise at a few test points;
  the log-marginal gradient 0.5 tr((alpha alpha^T - G) dK_y/dtheta) in the library's order [dl..., da, ds, dnoise]:
      dK/dlog l_d = k / (1 + w) (a_d - b_d)^2 / l_d^2 (an iso dl is the sum over d),
      dK/dlog alpha = k alpha (w / (1 + w) - log(1 + w)),  dK/dlog sigma = 2 K,  dK_y/dlog sigma_n = 2 noise I;
  the leave-one-out moments and density of GPML eqs. 5.10-5.12 (d = diag G) and the gradient of their sum, eq. 5.13 with the
      matrix M = (u alpha^T + alpha u^T) / 2 - G diag((1 + alpha_i^2 / d_i) / (2 d_i)) G, u = G (alpha / d);
  the input gradients dmu/dx_t = sum_i alpha_i dk_i, dvar/dx_t = -2 sum_i (G k*)_i dk_i with
      dk(x_t, x_i)/dx_{t,d} = -k / (1 + w) (x_{t,d} - x_{i,d}) / l_d^2.

Stored with each case: the kind, the inputs, a corner of K (up to 8 x 8) and the first rows of K(X, X*), cond_2(K_y) (4 digits:
tolerance metadata).  Before anything is written the n = 1 cases must agree with their closed forms, and for the n = 1, n = 2 and
the small D <= 3 cases every gradient must agree with mpmath's own numerical derivatives: mp.diff of the closed-form n <= 2
log-marginal, LOO density and predictive moments, and 50-digit central differences (step 1e-15, truncation ~1e-30) of the
log-marginal and the LOO density of the larger ones -- both independent of the contractions above.  Cases: duplicate training
points (w = 0 off the diagonal), the first test point on a training point in every case, length-scales spread over two decades,
alpha in {0.3, 2, 50}, D in {1, 3, 8}, the largest leaf at 300 rows.  Imports numpy and mpmath only (the data come from numpy's
PCG64 generator).  Run from the repo root:
    python tests/golden/make_rq_golden.py        (the cases run in parallel processes; a few minutes; byte-reproducible)
"""
import os
from multiprocessing import Pool

import mpmath as mp
import numpy as np

from mp_kernels import d_hyper, d_input, iso_logl as _iso, savez_reproducible, spread_logl as _logl, unpack, value

OUT = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
ISO, ARD = 9, 10
JIT = mp.mpf("1e-8")


def chol(kind, x, th):
    n, D = len(x), len(x[0])
    par = unpack(kind, th, D)
    c = mp.e ** (2 * th[-1]) + JIT
    L = []
    for i in range(n):
        row = []
        for j in range(i):
            row.append((value(kind, x[i], x[j], *par) - mp.fdot(row[:j], L[j][:j])) / L[j][j])
        row.append(mp.sqrt(value(kind, x[i], x[i], *par) + c - mp.fdot(row, row)))
        L.append(row)
    return L


def linv_columns(L):
    """Column j of L^-1 (rows j .. n-1) for every j."""
    n = len(L)
    cols = []
    for j in range(n):
        cj = [1 / L[j][j]]
        for i in range(j + 1, n):
            cj.append(-mp.fdot(L[i][j:i], cj) / L[i][i])
        cols.append(cj)
    return cols


def mll_lpd_of(kind, x, yc, th):
    """(log-marginal, summed LOO density) from the factor alone: what the central differences difference."""
    L = chol(kind, x, th)
    n = len(L)
    z = []
    for i in range(n):
        z.append((yc[i] - mp.fdot(L[i][:i], z)) / L[i][i])
    log2pi = mp.log(2 * mp.pi)
    mll = -(mp.fdot(z, z) + 2 * mp.fsum(mp.log(L[i][i]) for i in range(n)) + n * log2pi) / 2
    lpd = mp.mpf(0)
    for j, cj in enumerate(linv_columns(L)):
        d = mp.fdot(cj, cj)
        a = mp.fdot(cj, z[j:])
        lpd += -(log2pi - mp.log(d) + a * a / d) / 2
    return mll, lpd


def mp_case(kind, X, y, mean, th, Xt):
    n, D = X.shape
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    xt = [[mp.mpf(float(v)) for v in row] for row in Xt]
    par = unpack(kind, th, D)
    s2 = par[2]
    noise = mp.e ** (2 * th[-1])
    m = mp.mpf(float(mean))
    yc = [mp.mpf(float(v)) - m for v in y]
    L = chol(kind, x, th)
    cols = linv_columns(L)
    G = [[None] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            G[i][j] = G[j][i] = mp.fdot(cols[i], cols[j][i - j:])
    alpha = [mp.fdot(G[i], yc) for i in range(n)]
    log2pi = mp.log(2 * mp.pi)
    mll = -(mp.fdot(yc, alpha) + 2 * mp.fsum(mp.log(L[i][i]) for i in range(n)) + n * log2pi) / 2
    # leave-one-out moments, GPML eqs. 5.10-5.12
    d = [G[i][i] for i in range(n)]
    loo_var = [1 / d[i] for i in range(n)]
    loo_mu = [yc[i] + m - alpha[i] / d[i] for i in range(n)]
    lpd = [-(log2pi - mp.log(d[i]) + alpha[i] ** 2 / d[i]) / 2 for i in range(n)]
    # the two contraction matrices: W for the log-marginal, M for the LOO density
    u = [mp.fdot(G[i], [alpha[j] / d[j] for j in range(n)]) for i in range(n)]
    wv = [(1 + alpha[i] ** 2 / d[i]) / (2 * d[i]) for i in range(n)]
    Gw = [[G[i][j] * wv[j] for j in range(n)] for i in range(n)]
    nh = len(th) - 1
    gm = [mp.mpf(0)] * nh
    gl = [mp.mpf(0)] * nh
    trW = trM = mp.mpf(0)
    for i in range(n):
        for j in range(i + 1):
            Wij = alpha[i] * alpha[j] - G[i][j]
            Mij = (u[i] * alpha[j] + alpha[i] * u[j]) / 2 - mp.fdot(Gw[i], G[j])
            f = 1 if i == j else 2
            if i == j:
                trW += Wij
                trM += Mij
            dk = d_hyper(kind, x[i], x[j], *par)[1]
            for p in range(nh):
                gm[p] += f * Wij * dk[p] / 2
                gl[p] += f * Mij * dk[p]
    grad = gm + [noise * trW]
    loo_grad = gl + [2 * noise * trM]
    # predictive moments and their input gradients
    mu, var, dmu, dvar = [], [], [], []
    for t in range(len(xt)):
        ks = [value(kind, x[i], xt[t], *par) for i in range(n)]
        v = []
        for i in range(n):
            v.append((ks[i] - mp.fdot(L[i][:i], v)) / L[i][i])
        mu.append(m + mp.fdot(ks, alpha))
        var.append(s2 - mp.fdot(v, v) + noise)
        beta = [mp.fdot(G[i], ks) for i in range(n)]
        dk = [d_input(kind, xt[t], x[i], *par) for i in range(n)]
        dmu.append([mp.fdot(alpha, [dk[i][dd] for i in range(n)]) for dd in range(D)])
        dvar.append([-2 * mp.fdot(beta, [dk[i][dd] for i in range(n)]) for dd in range(D)])
    c = min(n, 8)
    Kc = np.array([[float(value(kind, x[i], x[j], *par)) for j in range(c)] for i in range(c)])
    Kt = np.array([[float(value(kind, x[i], xt[t], *par)) for t in range(len(xt))] for i in range(c)])
    Ky = np.array([[float(value(kind, x[i], x[j], *par)) for j in range(n)] for i in range(n)]) + float(noise + JIT) * np.eye(n)
    return dict(x=x, xt=xt, yc=yc, grad=grad, loo_grad=loo_grad, mll=mll, mu=mu, var=var, dmu=dmu, dvar=dvar, loo_mu=loo_mu,
                loo_var=loo_var, lpd=lpd, Kc=Kc, Kt=Kt, Ky=Ky)


def _small(kind, x, yc, m, th, xt=None):
    """n = 1 and n = 2 by hand (2 x 2 inverse written out): (mll, lpd sum), or (mu, var) at the test point xt."""
    D = len(x[0])
    par = unpack(kind, th, D)
    s2 = par[2]
    noise = mp.e ** (2 * th[-1])
    a = s2 + noise + JIT
    log2pi = mp.log(2 * mp.pi)
    if len(x) == 1:
        if xt is not None:
            k0 = value(kind, x[0], xt, *par)
            return m + k0 * yc[0] / a, s2 - k0 * k0 / a + noise
        v = -(yc[0] ** 2 / a + mp.log(a) + log2pi) / 2
        return v, v                                               # one point: the LOO density is the prior's
    b = value(kind, x[0], x[1], *par)
    det = a * a - b * b
    if xt is not None:
        k0, k1 = value(kind, x[0], xt, *par), value(kind, x[1], xt, *par)
        mu = m + (k0 * (a * yc[0] - b * yc[1]) + k1 * (a * yc[1] - b * yc[0])) / det
        return mu, s2 - (a * k0 * k0 - 2 * b * k0 * k1 + a * k1 * k1) / det + noise
    mll = -((a * yc[0] ** 2 - 2 * b * yc[0] * yc[1] + a * yc[1] ** 2) / det + mp.log(det) + 2 * log2pi) / 2
    al0, al1, d = (a * yc[0] - b * yc[1]) / det, (a * yc[1] - b * yc[0]) / det, a / det
    lpd = -(2 * log2pi - 2 * mp.log(d) + (al0 ** 2 + al1 ** 2) / d) / 2
    return mll, lpd


def _close(a, b, tol, what):
    assert abs(a - b) <= mp.mpf(tol) * max(1, abs(b)), (what, a, b)


def self_check(name, kind, r, m, th):
    """Closed forms and mpmath's own numerical derivatives (see the module docstring); raises before anything is written."""
    x, xt, yc = r["x"], r["xt"], r["yc"]
    n, D = len(x), len(x[0])
    nl = D if kind == ARD else 1
    if n <= 2:
        mll, lpd = _small(kind, x, yc, m, th)
        _close(r["mll"], mll, "1e-40", name + " mll")
        _close(mp.fsum(r["lpd"]), lpd, "1e-40", name + " lpd")
        for j in range(len(th)):
            for w, key in ((0, "grad"), (1, "loo_grad")):
                g = mp.diff(lambda t, j=j, w=w: _small(kind, x, yc, m, th[:j] + [t] + th[j + 1:])[w], th[j])
                _close(r[key][j], g, "1e-30", f"{name} {key}[{j}]")
        for t in range(len(xt)):
            mu, var = _small(kind, x, yc, m, th, xt[t])
            _close(r["mu"][t], mu, "1e-40", name + " mu")
            _close(r["var"][t], var, "1e-40", name + " var")
            for dd in range(D):
                for w, key in ((0, "dmu"), (1, "dvar")):
                    g = mp.diff(lambda v, dd=dd, w=w: _small(kind, x, yc, m, th, xt[t][:dd] + [v] + xt[t][dd + 1:])[w], xt[t][dd])
                    _close(r[key][t][dd], g, "1e-30", f"{name} {key}[{t}][{dd}]")
    if n == 1:         # K = sigma^2: no length-scale and no shape term; the LOO density is the log-marginal
        s2, noise = mp.e ** (2 * th[nl + 1]), mp.e ** (2 * th[-1])
        a = yc[0] / (s2 + noise + JIT)
        p = a * a - 1 / (s2 + noise + JIT)
        for key in ("grad", "loo_grad"):
            for got, want in zip(r[key], [mp.mpf(0)] * (nl + 1) + [p * s2, p * noise]):
                _close(got, want, "1e-40", name + " n=1 " + key)
        _close(r["loo_mu"][0], m, "1e-40", name + " n=1 loo mu")
        _close(r["loo_var"][0], s2 + noise + JIT, "1e-40", name + " n=1 loo var")
    if 2 < n <= 130 and D <= 3:
        step = mp.mpf("1e-15")
        for j in range(len(th)):
            hp, hm = list(th), list(th)
            hp[j] += step
            hm[j] -= step
            fp, fm = mll_lpd_of(kind, x, yc, hp), mll_lpd_of(kind, x, yc, hm)
            _close(r["grad"][j], (fp[0] - fm[0]) / (2 * step), "1e-24", f"{name} grad[{j}] vs differences")
            _close(r["loo_grad"][j], (fp[1] - fm[1]) / (2 * step), "1e-24", f"{name} loo_grad[{j}] vs differences")


# name, kind, n, D, logl, alpha, logs, logNoise, target offset (then the leaf's mean stays 0), duplicated rows
SPECS = [
    ("n1_iso_d3", ISO, 1, 3, _iso(3), 2.0, 0.1, np.log(0.2), 0.0, 0),
    ("n1_ard_d3", ARD, 1, 3, _logl(3), 0.3, 0.1, np.log(0.2), 0.0, 0),
    ("n2_iso_d3", ISO, 2, 3, _iso(3), 0.3, -0.2, np.log(0.2), 0.0, 0),
    ("n2_ard_d3", ARD, 2, 3, _logl(3), 2.0, -0.2, np.log(0.2), 0.0, 0),
    ("n2_ard_d1", ARD, 2, 1, _logl(1), 50.0, 0.3, np.log(0.3), 0.0, 0),
    ("n127_iso_d1", ISO, 127, 1, _iso(1), 2.0, 0.0, np.log(0.2), 0.0, 0),
    ("n127_ard_d1", ARD, 127, 1, _logl(1), 50.0, 0.0, np.log(0.2), 0.0, 0),
    ("n128_ard_d3", ARD, 128, 3, _logl(3), 0.3, 0.2, np.log(0.2), 0.0, 0),
    ("n128_iso_d3", ISO, 128, 3, _iso(3), 50.0, 0.2, np.log(0.2), 0.0, 0),
    ("n129_ard_d8", ARD, 129, 8, _logl(8), 50.0, 0.0, np.log(0.2), 0.0, 0),
    ("n129_iso_d8", ISO, 129, 8, _iso(8), 0.3, 0.0, np.log(0.2), 0.0, 0),
    ("n300_ard_d8", ARD, 300, 8, _logl(8), 2.0, -0.1, np.log(0.25), 0.0, 0),
    ("spread_ard_d8", ARD, 129, 8, np.log(np.geomspace(0.05, 5.0, 8)), 2.0, 0.0, np.log(0.2), 0.0, 0),
    ("dup_iso_d3", ISO, 140, 3, _iso(3), 50.0, 0.0, np.log(0.3), 0.0, 24),
    ("dup_ard_d3", ARD, 140, 3, _logl(3), 0.3, 0.0, np.log(0.3), 0.0, 24),
    ("offset_iso_d3", ISO, 128, 3, _iso(3), 2.0, 0.5, np.log(0.2), 3.0, 0),
]


def run_case(args):
    si, (name, kind, n, D, logl, alpha, logs, logNoise, offset, dup) = args
    mp.mp.dps = 50
    rng = np.random.Generator(np.random.PCG64(9000 + si))
    X = rng.random((n, D))
    if dup:            # the last `dup` rows repeat earlier ones: w = 0 off the diagonal
        X[n - dup:] = X[rng.choice(n - dup, dup, replace=False)]
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n) + offset
    Xt = rng.random((6, D))
    Xt[0] = X[n // 2]                                             # a test point on a training point
    mean = 0.0 if (n <= 2 or offset != 0.0) else float(np.mean(y))
    loga = float(np.log(alpha))
    th = [mp.mpf(float(v)) for v in logl] + [mp.mpf(loga), mp.mpf(float(logs)), mp.mpf(float(logNoise))]
    r = mp_case(kind, X, y, mean, th, Xt)
    self_check(name, kind, r, mp.mpf(mean), th)
    ev = np.linalg.eigvalsh(r["Ky"])
    cond = float(f"{ev[-1] / ev[0]:.4g}")
    f64 = lambda v: np.array([float(e) for e in v])               # noqa: E731
    rec = dict(kind=kind, X=X, y=y, Xt=Xt, mean=mean, logl=np.asarray(logl, dtype=np.float64), loga=loga, logs=float(logs),
               logNoise=float(logNoise), grad=f64(r["grad"]), loo_grad=f64(r["loo_grad"]), mll=float(r["mll"]),
               mu=f64(r["mu"]), var=f64(r["var"]), dmu=np.array([f64(v) for v in r["dmu"]]),
               dvar=np.array([f64(v) for v in r["dvar"]]), loo_mu=f64(r["loo_mu"]), loo_var=f64(r["loo_var"]),
               lpd=f64(r["lpd"]), lpd_sum=float(mp.fsum(r["lpd"])), Kc=r["Kc"], Kt=r["Kt"], cond=cond)
    print(f"{name:14s} kind {kind:2d} n {n:3d} D {D}  alpha {alpha:4g}  cond {cond:9.4g}  mll {rec['mll']:12.6g}  lpd {rec['lpd_sum']:12.6g}  "
          f"|g|inf {np.max(np.abs(rec['grad'])):9.3g}  |g_loo|inf {np.max(np.abs(rec['loo_grad'])):9.3g}", flush=True)
    return name, rec


def main():
    with Pool(min(len(SPECS), os.cpu_count() or 1)) as pool:
        res = pool.map(run_case, sorted(enumerate(SPECS), key=lambda a: -a[1][2]), chunksize=1)     # the largest leaf first
    flat = {}
    for name, rec in res:
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
    out = os.path.join(OUT, "gp_rq.npz")
    savez_reproducible(out, flat)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
