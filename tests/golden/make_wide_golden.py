"""Generate tests/golden/gp_predgrad_wide.npz and tests/golden/gp_predcov_wide.npz: the 50-digit references of the prediction-side
kernels past one chunk of input dimensions, with DISTINCT length-scales per dimension, so that a kernel that reads the factor of
another dimension (p.nh[d] in place of p.nh[d0 + d]) misses them by orders of magnitude (tests/test_wide_inputs_host.py shows it).

gp_predgrad_wide.npz -- input gradients of the predictive mean and variance, the layout and meta of gp_predgrad.npz
(predgrad_dense.case_inputs reads both): all eleven kinds (0-10) x D in {8, 9, 17, 36} at (n, n_t) = (130, 9).  The input-gradient
kernels work in chunks of 8 dimensions: D = 8 is exactly one chunk, 9 two rounds with a tail of one, 17 three rounds (a chunk
with rounds before and after it), 36 is past 32 and 35 (the limits of the fit and of the 35-dimension staging); n = 130 leaves a
second 128-row slab of 2 training rows, n_t = 9 live and dead rows in one test tile.  The inputs, targets, mean, noise and the
special rows are those of make_predgrad_golden.py (`inputs`, `run_case`: row 0 AT a training row, row 4 = row 1, rows 2 and 3
at +-1e3 for the stationary kinds other than the rational quadratic ones); the hyper-vectors are `wide_loghyp`.  Every case
passes run_case's checks: mp.diff of the 50-digit mu(x), sigma^2(x) along dimensions of the first, a middle and the last chunk
within 1e-12, cond_2(K_y) <= 1e6, and the float64 dense helper within predgrad_dense.tolerances of the 50 digits.

gp_predcov_wide.npz -- full predictive covariances, the layout and meta of gp_predcov.npz: (n, n_t) = (20, 130) at D = 36 (the
covariance epilogue stages coordinates in rounds of 35 dimensions; 130 rows give the tiles (0,0), (1,0), (1,1)), one kind per
device arm that reads the per-dimension factors: ArdSE 1, ArdLinear 3, ArdSEProduct 4, ArdMatern52 8, ArdRQ 10.  Test rows as
make_predcov_golden.py builds them (make_pred_golden.single_rows); the float64 dense GP must stay within the per-entry tolerance.

Both files stay below gp_pred.npz.  Run from the repo root:
    python tests/golden/make_wide_golden.py [predgrad|predcov]      (a few minutes on 8 cores; the output is byte-reproducible)
"""
import multiprocessing
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
import mp_kernels as mpk  # noqa: E402
import make_predcov_golden as mcov  # noqa: E402
import make_predgrad_golden as mgrad  # noqa: E402
from make_pred_golden import single_rows, uniform, normal  # noqa: E402

NAMES = mgrad.NAMES + ["isorq", "ardrq"]
WIDE_D = (8, 9, 17, 36)
N, NT = 130, 9
COV_KINDS = (1, 3, 4, 8, 10)
COV_N, COV_NT, COV_D = 20, 130, 36


def wide_loghyp(kind, D):
    """Hyper-vector without the noise: mp_kernels.spread_logl (distinct per dimension) for the ARD kinds, iso_logl for the others,
    + 0.5 on the scale for the linear kinds, alpha = 1.5 for the rational quadratic ones."""
    logl = mpk.spread_logl(D) if kind in dk.ARD else mpk.iso_logl(D)
    if kind in dk.LINEAR:
        logl = np.log(np.exp(logl) + 0.5)
    return dk.pack(kind, logl, 0.0 if kind in dk.LINEAR else 0.1, loga=np.log(1.5))


def grad_case(spec):
    _, kind, _, _, D = spec
    return mgrad.run_case(spec, loghyp=wide_loghyp(kind, D), diff_dims=sorted({0, min(8, D - 1), D - 1}))


def predgrad():
    flat = {}
    specs = [(f"{NAMES[kind]}_{N}_{NT}_{D}", kind, N, NT, D) for kind in range(11) for D in WIDE_D]
    for D in WIDE_D:
        X, y, Xt, _ = mgrad.inputs(N, NT, D)
        flat[f"in_{N}_{NT}_{D}/X"], flat[f"in_{N}_{NT}_{D}/y"], flat[f"in_{N}_{NT}_{D}/Xt"] = X, y, Xt
    specs.sort(key=lambda s: -s[4])
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, out, meta in pool.imap_unordered(grad_case, specs):
            flat[name + "/out"], flat[name + "/meta"] = out, meta
    return finish("gp_predgrad_wide.npz", flat)


def cov_case(item):
    mp.mp.dps = 50
    si, kind = item
    name = f"{NAMES[kind]}_d{COV_D}"
    n, R, D = COV_N, COV_NT, COV_D
    X = uniform(2100 + si, 0, n * D).reshape((n, D), order="F")
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, -1]) + 0.1 * normal(2150 + si, 0, n)
    mean = float(np.mean(y))
    loghyp, logNoise = wide_loghyp(kind, D), float(np.log(0.1))
    Xt, pos = single_rows(200 + si, kind if kind in dk.LINEAR else 0, X, R)
    dup = pos["dup"]
    g = mcov.MPCov(kind, loghyp, logNoise, X)
    low, kss_mp = g.cov(Xt)
    tr, tc = mcov.packed_lower(R)
    sig = np.array([float(low[(int(r), int(c))]) for r, c in zip(tr, tc)])
    kss = np.array([float(v) for v in kss_mp])
    S = np.zeros((R, R))
    S[tr, tc] = sig
    S[tc, tr] = sig
    So = mcov.oracle_cov(kind, loghyp, logNoise, X, y, mean, Xt)
    ratio = float(np.max(np.abs(So - S) / mcov.entry_tol(S, kss, float(g.noise))))
    assert ratio <= 1.0, (name, ratio)
    assert np.array_equal(S[dup[0]], S[dup[1]]), name
    rec = dict(X=X, y=y, Xt=Xt, loghyp=loghyp, sigma=sig, kss=kss,
               meta=np.array([kind, mean, logNoise, g.cond, dup[0], dup[1]], dtype=np.float64))
    print(f"{name:18s} kind {kind:2d} n {n:3d} rows {R:3d} D {D:2d}  cond {g.cond:9.4g}  dense err / tol {ratio:8.2g}", flush=True)
    return name, rec


def predcov():
    flat = {}
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, rec in pool.imap_unordered(cov_case, list(enumerate(COV_KINDS))):
            for k, v in rec.items():
                flat[f"{name}/{k}"] = np.asarray(v)
    return finish("gp_predcov_wide.npz", flat)


def finish(fname, flat):
    path = os.path.join(HERE, fname)
    mcov.savez_reproducible(path, flat)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "gp_pred.npz"))
    print(f"{path}: {size} bytes (gp_pred.npz: {limit})")
    assert size <= limit
    return path


if __name__ == "__main__":
    which = sys.argv[1:] or ["predgrad", "predcov"]
    assert set(which) <= {"predgrad", "predcov"}, which
    if "predgrad" in which:
        predgrad()
    if "predcov" in which:
        predcov()
