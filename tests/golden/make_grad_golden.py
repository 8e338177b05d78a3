"""Generate tests/golden/gp_grad.npz: 50-digit gradients of the log-marginal of single GP leaves.

Every case is evaluated in mpmath at 50 digits straight from the textbook equations: K, K_y = K + (noise + 1e-8) I, its
Cholesky factor L, alpha = K_y^-1 (y - mean), K_y^-1 = L^-T L^-1, and every gradient component as the direct contraction
0.5 tr((alpha alpha^T - K_y^-1) dK/dtheta) -- never through the identity tr(P K) = (y.alpha - c alpha.alpha) - (n - c tr K_y^-1)
the device uses.  The components are stored in the library's convention (src/gaussianprocess.jl:212-214: [dl..., ds, dnoise]):

  IsoSE      dl and ds carry the reference's extra factor sigma (src/kernels.jl:90-97)
  ArdSE      dl = 0 (src/kernels.jl:161); the true d/dlog l_d is stored as `grad_true`
  IsoLinear  dl = 0.5 tr(P (-2 K)) (src/kernels.jl:198), 0 in the variance slot
  ArdLinear  the true d/dlog l_d, 0 in the variance slot (include/dsmgp_hip.h, DSMGP_KIND_ARD_LINEAR)

together with the log-marginal, cond_2(K_y) and, for the tolerance of the weak-signal cases, n and c tr K_y^-1.  Before
anything is stored the oracle (oracle.gp, tests/dense_gp.DenseGP for ArdLinear) must agree with the 50-digit values,
and the n = 1 and n = 2 cases must agree with their closed forms.  Imports: oracle/, datagen and tests/dense_gp.py
only.  Run from the repo root:  python tests/golden/make_grad_golden.py   (about a minute; the output is byte-reproducible)
"""
import importlib.util
import io
import os
import sys
import zipfile

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import gp as ogp  # noqa: E402
from dense_gp import DenseGP  # noqa: E402

# the data generator alone, loaded from its file: importing it through the package would run the product's model and tree code
_spec = importlib.util.spec_from_file_location("datagen", os.path.join(ROOT, "deepstructuredmixtures_amd", "datagen.py"))
datagen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(datagen)
uniform, normal = datagen.uniform, datagen.normal

OUT = os.path.dirname(os.path.abspath(__file__))
mp.mp.dps = 50
EPS = np.finfo(np.float64).eps


def _lt(P, M):
    """sum_ij P_ij M_ij of two symmetric matrices held as lower triangles (rows i: entries j <= i)."""
    s = mp.mpf(0)
    for i in range(len(P)):
        s += 2 * mp.fdot(P[i][:i], M[i][:i]) + P[i][i] * M[i][i]
    return s


def mp_grad(kind, loghyp, logNoise, X, y, mean):
    """50-digit (grad [library convention], grad_true [per-dimension d/dlog l_d, ArdSE only], mll, K_y rounded, c tr K_y^-1)."""
    n, D = X.shape
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    h = [mp.mpf(float(v)) for v in loghyp]
    noise = mp.e ** (2 * mp.mpf(float(logNoise)))
    c = noise + mp.mpf("1e-8")
    # K and the derivatives dK/dtheta for every length-scale / variance parameter theta, lower triangles
    dK = []
    if kind == 0:
        l2, s2 = mp.e ** (2 * h[0]), mp.e ** (2 * h[1])
        K, Kl = [], []
        for i in range(n):
            row, rowl = [], []
            for j in range(i + 1):
                u = [x[i][d] - x[j][d] for d in range(D)]
                r = mp.fdot(u, u)
                k = s2 * mp.e ** (-r / (2 * l2))
                row.append(k)
                rowl.append(k * r / l2)
            K.append(row)
            Kl.append(rowl)
        dK = [Kl, [[2 * k for k in row] for row in K]]
    elif kind == 1:
        l2 = [mp.e ** (2 * v) for v in h[:D]]
        s2 = mp.e ** (2 * h[D])
        K = []
        Kd = [[] for _ in range(D)]
        for i in range(n):
            row = []
            rows = [[] for _ in range(D)]
            for j in range(i + 1):
                tot = mp.mpf(0)
                for d in range(D):
                    q = (x[i][d] - x[j][d]) ** 2 / l2[d]
                    e = s2 * mp.e ** (-q / 2)
                    tot += e
                    rows[d].append(e * q)
                row.append(tot)
            K.append(row)
            for d in range(D):
                Kd[d].append(rows[d])
        dK = Kd + [[[2 * k for k in row] for row in K]]
    elif kind == 2:
        l2 = mp.e ** (2 * h[0])
        K = [[mp.fdot(x[i], x[j]) / l2 for j in range(i + 1)] for i in range(n)]
        dK = [[[-2 * k for k in row] for row in K]]
    else:
        il2 = [1 / mp.e ** (2 * v) for v in h[:D]]
        K = [[mp.fdot([x[i][d] * x[j][d] for d in range(D)], il2) for j in range(i + 1)] for i in range(n)]
    Ky = [[K[i][j] + (c if i == j else 0) for j in range(i + 1)] for i in range(n)]
    # Cholesky factor (rows), W = L^-1 (columns: col[j][k - j] = W[k][j]), K_y^-1 = W^T W (lower triangle)
    L = []
    for i in range(n):
        row = []
        for j in range(i):
            row.append((Ky[i][j] - mp.fdot(row[:j], L[j][:j])) / L[j][j])
        row.append(mp.sqrt(Ky[i][i] - mp.fdot(row, row)))
        L.append(row)
    col = []
    for j in range(n):
        cj = [1 / L[j][j]]
        for i in range(j + 1, n):
            cj.append(-mp.fdot(L[i][j:i], cj) / L[i][i])
        col.append(cj)
    Kinv = [[mp.fdot(col[i], col[j][i - j:]) for j in range(i + 1)] for i in range(n)]
    yc = [mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y]
    full = lambda A, i, j: A[i][j] if j <= i else A[j][i]      # noqa: E731
    alpha = [mp.fdot([full(Kinv, i, j) for j in range(n)], yc) for i in range(n)]
    P = [[alpha[i] * alpha[j] - Kinv[i][j] for j in range(i + 1)] for i in range(n)]
    trP = sum(P[i][i] for i in range(n))
    trKinv = sum(Kinv[i][i] for i in range(n))
    mll = -(mp.fdot(yc, alpha) + 2 * sum(mp.log(L[i][i]) for i in range(n)) + n * mp.log(2 * mp.pi)) / 2
    dnoise = noise * trP                                    # 0.5 tr(P dK_y/dlog sigma_n), dK_y = 2 noise I
    grad_true = None
    if kind == 0:
        sigma = mp.e ** h[1]
        grad = [sigma * _lt(P, dK[0]) / 2, sigma * _lt(P, dK[1]) / 2, dnoise]
    elif kind == 1:
        sigma = mp.e ** h[D]
        grad_true = [_lt(P, dK[d]) / 2 for d in range(D)]
        grad = [mp.mpf(0)] * D + [sigma * _lt(P, dK[D]) / 2, dnoise]
    elif kind == 2:
        grad = [_lt(P, dK[0]) / 2, mp.mpf(0), dnoise]
    else:
        # dK/dlog l_d = -2 x_d x_d^T / l_d^2: 0.5 tr(P dK) = -(x_d^T P x_d) / l_d^2, P contracted entry by entry
        grad = []
        for d in range(D):
            xd = [x[i][d] for i in range(n)]
            Pxd = [mp.fdot([full(P, i, j) for j in range(n)], xd) for i in range(n)]
            grad.append(-mp.fdot(xd, Pxd) * il2[d])
        grad += [mp.mpf(0), dnoise]
    Kyf = np.array([[float(full(Ky, i, j)) for j in range(n)] for i in range(n)])
    return grad, grad_true, mll, Kyf, c * trKinv


def closed_form(name, kind, loghyp, logNoise, X, y, mean):
    """n = 1 (IsoSE, IsoLinear) and n = 2 (IsoSE) gradients written out by hand, at 50 digits."""
    noise = mp.e ** (2 * mp.mpf(float(logNoise)))
    c = noise + mp.mpf("1e-8")
    yc = [mp.mpf(float(v)) - mp.mpf(float(mean)) for v in y]
    x = [[mp.mpf(float(v)) for v in row] for row in X]
    if X.shape[0] == 1:
        k = mp.e ** (2 * mp.mpf(float(loghyp[1]))) if kind == 0 else mp.fdot(x[0], x[0]) / mp.e ** (2 * mp.mpf(float(loghyp[0])))
        a = yc[0] / (k + c)
        p = a * a - 1 / (k + c)
        if kind == 0:          # r = 0: no length-scale term; ds = sigma * p * s2
            return [mp.mpf(0), mp.e ** mp.mpf(float(loghyp[1])) * p * k, noise * p]
        return [-p * k, mp.mpf(0), noise * p]
    # n = 2, IsoSE: K_y = [[a, b], [b, a]]
    sigma, l2 = mp.e ** mp.mpf(float(loghyp[1])), mp.e ** (2 * mp.mpf(float(loghyp[0])))
    s2 = sigma ** 2
    r = sum((x[0][d] - x[1][d]) ** 2 for d in range(X.shape[1]))
    a, b = s2 + c, s2 * mp.e ** (-r / (2 * l2))
    det = a * a - b * b
    al = [(a * yc[0] - b * yc[1]) / det, (a * yc[1] - b * yc[0]) / det]
    P00, P11, P01 = al[0] ** 2 - a / det, al[1] ** 2 - a / det, al[0] * al[1] + b / det
    return [sigma * P01 * b * r / l2, sigma * ((P00 + P11) * s2 + 2 * P01 * b), noise * (P00 + P11)]


# name, kind, n, D, loghyp (library hyper-vector without the noise), logNoise, weak signal
SQ = np.sqrt
SPECS = [
    ("isose_n1", 0, 1, 2, [np.log(0.5), 0.1], np.log(0.2), False),
    ("isolinear_n1", 2, 1, 2, [np.log(0.8), 0.0], np.log(0.2), False),
    ("isose_n2", 0, 2, 1, [np.log(0.6), -0.2], np.log(0.2), False),
    ("isose_n127", 0, 127, 3, [np.log(0.4), 0.0], np.log(0.2), False),
    ("isose_n128", 0, 128, 3, [np.log(0.4), 0.0], np.log(0.2), False),
    ("isose_n129", 0, 129, 3, [np.log(0.4), 0.0], np.log(0.2), False),
    ("isose_d35", 0, 160, 35, [np.log(0.3 * SQ(35)), 0.0], np.log(0.2), False),
    ("isose_d36", 0, 160, 36, [np.log(0.3 * SQ(36)), 0.0], np.log(0.2), False),
    ("isose_d48", 0, 160, 48, [np.log(0.3 * SQ(48)), 0.0], np.log(0.2), False),
    ("ardse_d3", 1, 129, 3, list(np.log([0.4, 0.6, 0.9])) + [-0.3], np.log(0.2), False),
    ("ardse_d35", 1, 160, 35, list(np.log(np.linspace(0.3, 1.2, 35))) + [-0.5 * np.log(35.0)], np.log(0.2), False),
    ("isolinear_n160", 2, 160, 3, [np.log(1.0), 0.0], np.log(0.2), False),
    ("ardlinear_d5", 3, 160, 5, list(np.log(np.linspace(0.8, 1.6, 5))) + [0.0], np.log(0.2), False),
    ("ardlinear_d36", 3, 160, 36, list(np.log(SQ(36) * np.linspace(0.8, 1.6, 36))) + [0.0], np.log(0.2), False),
    # weak signal: sigma^2 / c = 1e-8 (IsoLinear: the mean prior variance D E[x^2] / l^2 = (2/3) / l^2), data at noise level
    ("isose_weak", 0, 160, 2, [np.log(0.4), 0.5 * np.log(1e-8 * (0.04 + 1e-8))], np.log(0.2), True),
    ("isolinear_weak", 2, 160, 2, [0.5 * np.log((2.0 / 3.0) / (1e-8 * (0.04 + 1e-8))), 0.0], np.log(0.2), True),
]


def oracle_grad(kind, loghyp, logNoise, X, y, mean):
    if kind == 3:
        g = DenseGP(3, np.append(loghyp, logNoise), X, y, mean)
        return g, g.grad()
    g = ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, loghyp), logNoise, exact_dist=True).update_cholesky()
    return g, g.grad()


def savez_reproducible(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


def main():
    flat = {}
    for si, (name, kind, n, D, loghyp, logNoise, weak) in enumerate(SPECS):
        X = uniform(900 + si, 0, n * D).reshape((n, D), order="F")
        y = 0.2 * normal(950 + si, 0, n) if weak else np.sin(3.0 * X[:, 0]) + 0.1 * normal(950 + si, 0, n)
        mean = float(np.mean(y)) if n > 2 else 0.0          # n = 1: y - mean(y) would be zero
        loghyp = np.array(loghyp, dtype=np.float64)
        grad, grad_true, mll, Ky, ctr = mp_grad(kind, loghyp, logNoise, X, y, mean)
        ev = np.linalg.eigvalsh(Ky)
        cond = float(f"{ev[-1] / ev[0]:.4g}")            # tolerance metadata: 4 digits, stable across LAPACK builds
        g = np.array([float(v) for v in grad])
        if n <= 2:
            cf = closed_form(name, kind, loghyp, logNoise, X, y, mean)
            for a, b in zip(grad, cf):
                assert abs(a - b) <= mp.mpf("1e-40") * max(1, abs(b)), (name, a, b)
        # the f64 oracle must agree with the 50-digit values before anything is stored
        go, vo = oracle_grad(kind, loghyp, logNoise, X, y, mean)
        tol = 16 * cond * EPS * max(1.0, float(np.max(np.abs(g))))
        assert go.info == 0, name
        assert np.max(np.abs(vo - g)) <= tol, (name, vo, g, tol)
        assert abs(go.mll() - float(mll)) <= 16 * cond * EPS * max(1.0, abs(float(mll))), (name, go.mll(), float(mll))
        if grad_true is not None:
            # the true ArdSE length-scale gradient has no oracle: central differences of the oracle's log-marginal
            e = 1e-5
            for d in range(D):
                hp, hm = loghyp.copy(), loghyp.copy()
                hp[d] += e
                hm[d] -= e
                fd = (oracle_grad(1, hp, logNoise, X, y, mean)[0].mll() - oracle_grad(1, hm, logNoise, X, y, mean)[0].mll()) / (2 * e)
                assert abs(fd - float(grad_true[d])) <= 1e-6 * max(1.0, abs(fd)), (name, d, fd, float(grad_true[d]))
        rec = dict(kind=kind, X=X, y=y, mean=mean, loghyp=loghyp, logNoise=logNoise, grad=g, mll=float(mll), cond=cond,
                   n=n, c_trKinv=float(ctr), weak=weak)
        if grad_true is not None:
            rec["grad_true"] = np.array([float(v) for v in grad_true])
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
        print(f"{name:16s} kind {kind} n {n:3d} D {D:2d}  cond {cond:9.4g}  |g|inf {np.max(np.abs(g)):9.3g}  "
              f"oracle err {np.max(np.abs(vo - g)):8.2g} (tol {tol:.2g})", flush=True)
    savez_reproducible(os.path.join(OUT, "gp_grad.npz"), flat)


if __name__ == "__main__":
    main()
