"""Generate tests/golden/gp_predcov.npz: 50-digit full predictive covariances of single leaves.

prediction(gp, xtest) of the reference returns the full Sigma = K_tt - V'V + noise I, V = L^-1 K_nt
(src/gaussianprocess.jl:110-137).  Everything is evaluated in mpmath at 50 digits from the float64 inputs the device reads:
the kernel matrix, K_y = K + (noise + 1e-8) I, its Cholesky factor, V row by row, and the lower triangle of Sigma WITHOUT the
noise, packed column by column: `sigma` lists (r, c) for c = 0 .. nt-1, r = c .. nt-1 (`packed_lower`).

Cases (test rows built like the single/ cases of gp_pred.npz: rows AT training inputs on both sides of a 128 edge, rows 1e-7
away, far rows, one row listed twice):
  every kernel kind (0-8) once at n and nt just above 128 -- two row tiles of test rows, so the tiles (0,0), (1,0), (1,1) of
  Sigma exist; n varies over the residues mod 8 (the device sums the last n % 8 columns outside its matrix loop);
  one n < 128, nt < 128; one nt = 1; one D > 35 (the coordinates are staged in two rounds).  The iso kinds have D = 1, the ARD
  kinds D = 2, and the three small cases are small: the packed triangles of the nine two-tile cases alone are 0.6 MB of
  incompressible doubles, and the file stays below the largest fixture committed before it (gp_pred.npz).

Before anything is stored every case is checked against the float64 oracle -- oracle.gp prediction(full_cov=True) for kinds
0-2, the dense GP of tests/dense_gp.py for the others -- to the variance
tolerance of tests/pred_tolerance.moment_tol applied per entry:  RTOL |Sigma_rc| + ATOL max(1, max(kss_r, kss_c) + noise).
Run from the repo root:  python tests/golden/make_predcov_golden.py   (a few minutes; the output is byte-reproducible)
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

from oracle import gp as ogp  # noqa: E402
from dense_gp import DenseGP  # noqa: E402
from pred_tolerance import RTOL, ATOL  # noqa: E402
import io  # noqa: E402
import zipfile  # noqa: E402

from make_pred_golden import single_rows, uniform, normal  # noqa: E402
import mp_kernels as mpk  # noqa: E402

mp.mp.dps = 50
SQ = np.sqrt


def savez_reproducible(path, arrays):
    """make_pred_golden.savez_reproducible at the highest deflate level: fixed member timestamps, a rerun writes the same bytes."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def packed_lower(nt):
    """(rows, columns) of the packed lower triangle, column by column."""
    c, r = np.triu_indices(nt)          # row-major upper = column-major lower with the roles swapped
    return r, c


def entry_tol(S, kss, noise):
    """moment_tol's variance tolerance per entry (r, c): sigma^2 is the r = c case of the same difference k - v_r.v_c, and
    |v_r.v_c| <= sqrt(kss_r kss_c) <= max(kss_r, kss_c)."""
    scale = np.maximum(kss[:, None], kss[None, :]) + noise
    return RTOL * np.abs(S) + ATOL * np.maximum(1.0, scale)


class MPCov:
    """One leaf at 50 digits, any kernel kind of include/dsmgp_hip.h (0-10); loghyp = the library hyper-vector without the noise."""

    def __init__(self, kind, loghyp, logNoise, X):
        self.kind = kind
        self.X = np.asarray(X, dtype=np.float64)
        n, D = self.X.shape
        h = [mp.mpf(float(v)) for v in loghyp]
        self.noise = mp.e ** (2 * mp.mpf(float(logNoise)))
        ard = kind in mpk.ARD
        nl = D if ard else 1
        il2 = [1 / mp.e ** (2 * v) for v in h[:nl]]
        self.il2 = il2 if ard else il2 * D
        self.s2 = mp.mpf(1) if kind in (2, 3) else mp.e ** (2 * h[nl])
        if kind in mpk.RQ:          # [logl..., loga, logs]: the table of mp_kernels
            self.il2, self.al, self.s2 = mpk.unpack(kind, h, D)
        self.x = [self.row(r) for r in self.X]
        c = self.noise + mp.mpf("1e-8")
        K = [[self.k(self.x[i], self.x[j]) for j in range(i + 1)] for i in range(n)]
        L = []
        for i in range(n):
            row = []
            for j in range(i):
                row.append((K[i][j] - mp.fdot(row[:j], L[j][:j])) / L[j][j])
            row.append(mp.sqrt(K[i][i] + c - mp.fdot(row, row)))
            L.append(row)
        self.L = L
        Ky = np.array([[float(K[max(i, j)][min(i, j)] + (c if i == j else 0)) for j in range(n)] for i in range(n)])
        ev = np.linalg.eigvalsh(Ky)
        self.cond = float(f"{ev[-1] / ev[0]:.4g}")

    @staticmethod
    def row(r):
        return [mp.mpf(float(v)) for v in r]

    def k(self, a, b):
        kind = self.kind
        if kind in mpk.RQ:
            return mpk.value(kind, a, b, self.il2, self.al, self.s2)
        if kind == 1:
            return self.s2 * mp.fsum(mp.e ** (-((p - q) ** 2) * il / 2) for p, q, il in zip(a, b, self.il2))
        if kind in (2, 3):
            return mp.fsum(p * q * il for p, q, il in zip(a, b, self.il2))
        r2 = mp.fsum((p - q) ** 2 * il for p, q, il in zip(a, b, self.il2))
        if kind in (0, 4):
            return self.s2 * mp.e ** (-r2 / 2)
        nu2 = 3 if kind in (5, 7) else 5
        s = mp.sqrt(nu2 * r2)
        return self.s2 * mp.e ** (-s) * (1 + s + (s * s / 3 if nu2 == 5 else 0))

    def cov(self, Xt):
        """(lower triangle of K_tt - V'V as {(r, c): value}, kss) at 50 digits."""
        xs = [self.row(r) for r in Xt]
        n = len(self.x)
        V = []
        for x in xs:
            ks = [self.k(xi, x) for xi in self.x]
            v = []
            for i in range(n):
                v.append((ks[i] - mp.fdot(self.L[i][:i], v)) / self.L[i][i])
            V.append(v)
        kss = [self.k(x, x) for x in xs]
        low = {}
        for r in range(len(xs)):
            for c in range(r + 1):
                low[(r, c)] = (kss[r] if r == c else self.k(xs[r], xs[c])) - mp.fdot(V[r], V[c])
        return low, kss


def oracle_cov(kind, loghyp, logNoise, X, y, mean, Xt):
    """Sigma without noise from the float64 oracle of the kind."""
    if kind <= 2:
        g = ogp.GaussianProcess(X, y, mean, ogp.make_kernel(kind, loghyp), logNoise, exact_dist=True).update_cholesky()
        assert g.info == 0
        _, S = g.prediction(Xt, full_cov=True)
        S = S.copy()
        S[np.diag_indices(Xt.shape[0])] -= g.getnoise()
        return S
    g = DenseGP(kind, np.append(loghyp, logNoise), X, y, mean)
    assert g.info == 0
    return g.prediction_cov(Xt, with_noise=False)


# name, kind, n, routed rows, D, loghyp (library hyper-vector without the noise), logNoise
CASES = [
    ("isose", 0, 130, 129, 1, [np.log(0.2), 0.0], np.log(0.1)),
    ("ardse", 1, 131, 129, 2, list(np.log([0.4, 0.6])) + [-0.2], np.log(0.1)),
    ("isolinear", 2, 132, 129, 1, [np.log(0.9), 0.0], np.log(0.1)),
    ("ardlinear", 3, 133, 129, 2, list(np.log([0.5, 0.8])) + [0.0], np.log(0.1)),
    ("ardseproduct", 4, 134, 129, 2, list(np.log([0.3, 0.45])) + [0.1], np.log(0.1)),
    ("isomatern32", 5, 135, 129, 1, [np.log(0.5), 0.0], np.log(0.1)),
    ("isomatern52", 6, 136, 129, 1, [np.log(0.5), 0.1], np.log(0.1)),
    ("ardmatern32", 7, 129, 129, 2, list(np.log([0.5, 0.8])) + [0.0], np.log(0.1)),
    ("ardmatern52", 8, 137, 129, 2, list(np.log([0.5, 0.8])) + [-0.1], np.log(0.1)),
    ("isose_small", 0, 40, 16, 2, [np.log(0.35), 0.0], np.log(0.1)),
    ("isose_nt1", 0, 23, 1, 2, [np.log(0.35), 0.0], np.log(0.1)),
    ("isose_d36", 0, 20, 10, 36, [np.log(0.3 * SQ(36)), 0.0], np.log(0.1)),
]


def main():
    flat = {}
    for si, (name, kind, n, R, D, loghyp, logNoise) in enumerate(CASES):
        X = uniform(2000 + si, 0, n * D).reshape((n, D), order="F")
        y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * normal(2050 + si, 0, n)
        mean = float(np.mean(y))
        loghyp = np.array(loghyp, dtype=np.float64)
        if R == 1:      # one row, 1e-7 away from a training input; no pair to list twice
            Xt = (X[n - 1] + 1e-7).reshape(1, D)
            dup = [0, 0]
        else:           # the far rows of the linear kinds are the origin and a large row, of every other kind +-1e3
            Xt, pos = single_rows(100 + si, kind if kind in (2, 3) else 0, X, R)
            dup = pos["dup"]
        g = MPCov(kind, loghyp, logNoise, X)
        low, kss_mp = g.cov(Xt)
        nt = Xt.shape[0]
        tr, tc = packed_lower(nt)
        sig = np.array([float(low[(int(r), int(c))]) for r, c in zip(tr, tc)])
        kss = np.array([float(v) for v in kss_mp])
        S = np.zeros((nt, nt))
        S[tr, tc] = sig
        S[tc, tr] = sig
        noise = float(g.noise)
        So = oracle_cov(kind, loghyp, logNoise, X, y, mean, Xt)
        ratio = float(np.max(np.abs(So - S) / entry_tol(S, kss, noise)))
        assert ratio <= 1.0, (name, ratio)
        assert np.array_equal(S[dup[0]], S[dup[1]]), name           # the row listed twice
        # the scalars of a case in one member (`meta`: kind, mean, logNoise, cond, the pair of the row listed twice): a zip member
        # costs ~300 bytes of headers, and the file has to stay below gp_pred.npz
        rec = dict(X=X, y=y, Xt=Xt, loghyp=loghyp, sigma=sig, kss=kss,
                   meta=np.array([kind, mean, logNoise, g.cond, dup[0], dup[1]], dtype=np.float64))
        for k, v in rec.items():
            flat[f"{name}/{k}"] = np.asarray(v)
        print(f"{name:13s} kind {kind} n {n:3d} rows {nt:3d} D {D:2d}  cond {g.cond:9.4g}  oracle err / tol {ratio:8.2g}", flush=True)
    out = os.path.join(HERE, "gp_predcov.npz")
    savez_reproducible(out, flat)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
