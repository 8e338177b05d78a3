"""Generate tests/golden/gp_sharing.npz: 50-digit references for the observation sets of tests/sharing_tables.py.

One entry per keyed set of at most 512 rows (sharing_tables.Data.mp_keys: every PREFIX leaf's own set and its source's, the
COPY leaves' with their own means): the log-marginal, alpha = K_y^-1 (y - mean), cond_2(K_y) (4 digits: tolerance metadata) and,
at the set's routed test rows, mu, sigma^2 and k(x*, x*) -- the arithmetic of make_pred_golden.MPLeaf (imported), with
ArdMatern52 and ArdRQ added to its kernel function as include/dsmgp_hip.h defines them:
    ArdMatern52   s = sqrt(5 sum_d (a_d - b_d)^2 / l_d^2),  k = sigma^2 (1 + s + s^2 / 3) e^-s
    ArdRQ         w = sum_d (a_d - b_d)^2 / (2 alpha l_d^2),  k = sigma^2 (1 + w)^-alpha
Sets above 512 rows get no entry: tests/test_sharing_gpu.py checks those leaves against the float64 oracle only.

Before anything is stored every entry is checked against the float64 oracle of its kind (sharing_tables.oracle_leaf) the way
make_pred_golden.table checks its own: moments and log-marginal within 16 cond_2(K_y) eps.  Run from the repo root:
    python tests/golden/make_sharing_golden.py     (the sets run in parallel processes; a few minutes; byte-reproducible)
"""
import os
import sys
from multiprocessing import Pool

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_pred_golden import MPLeaf, check_moments, f, savez_reproducible  # noqa: E402
import sharing_tables as st  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps


class SharingLeaf(MPLeaf):
    """MPLeaf with kinds 8 (ArdMatern52) and 10 (ArdRQ): MPLeaf reads the D length-scales of any ARD kind; the signal variance
    and the shape are read here."""

    def __init__(self, kind, loghyp, logNoise, X, targets):
        D = np.asarray(X).shape[1]
        h = [mp.mpf(float(v)) for v in loghyp]
        if kind == 8:
            self.sig2 = mp.e ** (2 * h[D])
        elif kind == 10:
            self.shape = mp.e ** h[D]
            self.sig2 = mp.e ** (2 * h[D + 1])
        super().__init__(kind, loghyp, logNoise, X, targets)

    def k(self, a, b):
        if self.kind not in (8, 10):
            return super().k(a, b)
        q = mp.fdot([(p - r) ** 2 for p, r in zip(a, b)], self.il2)
        if self.kind == 8:
            s = mp.sqrt(5 * q)
            return self.sig2 * (1 + s + s * s / 3) * mp.e ** (-s)
        return self.sig2 * mp.e ** (-self.shape * mp.log(1 + q / (2 * self.shape)))


def run_set(key):
    mp.mp.dps = 50
    dat = st.data(3)
    s = dat.sets[key]
    kind, hyp = st.KINDS[s["kid"]], st.hyper(s["kid"], dat.D)
    X, y, Xt = dat.X[s["obs"]], dat.y[s["obs"]], dat.Xt[s["rows"]]
    g = SharingLeaf(kind, hyp[:-1], hyp[-1], X, [(y, s["mean"])])
    res = [g.predict(r) for r in Xt]
    mu, var, kss = f([r[0][0] for r in res]), f([r[1] for r in res]), f([r[2] for r in res])
    mll = float(g.mll[0])
    go = st.oracle_leaf(kind, hyp, X, y, s["mean"])
    assert go.info == 0, key
    emu = evar = 0.0
    if Xt.shape[0]:
        mo, vo = go.prediction(Xt)
        emu, evar = check_moments(key, g.cond, mu, var, mo, vo, max(1.0, float(np.max(np.abs(y)))))
        assert np.allclose(st.prior_diag(kind, hyp, Xt), kss, rtol=4 * dat.D * EPS, atol=0), key
    emll = abs(go.mll() - mll) / max(1.0, abs(mll))
    assert emll <= 16 * g.cond * EPS, (key, emll)
    tol = 16 * g.cond * EPS
    print(f"{key:18s} kind {kind:2d} n {X.shape[0]:3d} rows {Xt.shape[0]:3d}  cond {g.cond:9.4g}  mll {mll:14.8g}  oracle err / tol: "
          f"mu {emu / tol:7.2g} var {evar / tol:7.2g} mll {emll / tol:7.2g}", flush=True)
    return key, dict(mll=mll, alpha=f(g.alpha[0]), cond=g.cond, mu=mu, var=var, kss=kss)


def main():
    keys = sorted(st.data(3).mp_keys(), key=lambda k: -st.data(3).sets[k]["obs"].size)      # the largest set first
    with Pool(min(len(keys), os.cpu_count() or 1)) as pool:
        res = pool.map(run_set, keys, chunksize=1)
    flat = {}
    for key, rec in res:
        for k, v in rec.items():
            flat[f"{key}/{k}"] = np.asarray(v)
    out = os.path.join(OUT, "gp_sharing.npz")
    savez_reproducible(out, flat)
    print(f"{out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
