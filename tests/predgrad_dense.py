"""Dense float64 input gradients of the predictive moments of one GP, and the tolerances of the predict-gradient tests.

For one leaf with training inputs X, K_y = K + (noise + 1e-8) I (the matrix the fit factorises), alpha = K_y^-1 (y - m) and,
per test row t, k_t = k(X, x_t), beta_t = K_y^-1 k_t:
    mu = m + k_t . alpha                      dmu[t, d]  = sum_i alpha_i dk(x_t, x_i) / dx_{t,d}
    var = k(x_t, x_t) - k_t . beta_t + noise  dvar[t, d] = dk(x_t, x_t) / dx_{t,d} - 2 sum_i beta_{t,i} dk(x_t, x_i) / dx_{t,d}
with the kernel derivatives of dense_kernels.d_input, every kind.  `loghyp` is the library hyper-vector without the noise:
[logl..., (loga,) logs] (the variance slot of the linear kinds is a dummy)."""
import numpy as np

from dense_gp import DenseGP
from dense_kernels import LINEAR, RQ, grad_scale, prior_diag
from pred_tolerance import RTOL, ATOL


def moments(kind, loghyp, logNoise, X, y, mean, Xt, L=None, alpha=None):
    """(mu, var, dmu, dvar) of one leaf in dense float64.  `L` (lower factor of K_y) and `alpha` may be given (the device's own,
    `Context.download_factor`); else they are DenseGP's."""
    g = DenseGP(kind, np.append(loghyp, logNoise), np.atleast_2d(X), y, mean, F=L, alpha=alpha)
    return g.prediction(Xt) + g.input_gradients(Xt)


def tolerances(kind, loghyp, logNoise, X, y, Xt, dmu, dvar):
    """(tol_dmu, tol_dvar) per entry: the north star RTOL relative, plus ATOL times the quantity's own scale --
    max(1, max|y|) g_d for dmu, max(1, k** + noise) g_d for dvar (pred_tolerance.moment_tol's scales times g_d)."""
    g = grad_scale(kind, loghyp, X, Xt)
    noise = float(np.exp(2.0 * logNoise))
    yscale = max(1.0, float(np.max(np.abs(y))))
    vscale = np.maximum(1.0, prior_diag(kind, loghyp, Xt) + noise)[:, None]
    return RTOL * np.abs(dmu) + ATOL * yscale * g, RTOL * np.abs(dvar) + ATOL * vscale * g


def case_inputs(z, name):
    """One single-leaf case of tests/golden/gp_predgrad.npz as the tests use it.  Cases of one (n, n_t, D) share the stored inputs
    `in_<n>_<nt>_<D>/{X, y, Xt}`; for the stationary kinds with n_t > 4 rows 2 and 3 of Xt are put at +-1e3 (the rule of
    tests/golden/make_predgrad_golden.py; not for the rational quadratic kinds, whose tails do not underflow).  meta = kind, n, n_t, D, mean, logNoise, cond, the pair of the row listed twice, then
    the hyper-vector without the noise; out = dmu | dvar (n_t x 2 D)."""
    m = z[name + "/meta"]
    kind, n, nt, D = (int(v) for v in m[:4])
    g = f"in_{n}_{nt}_{D}"
    Xt = np.array(z[g + "/Xt"], order="F")
    far = []
    if kind not in LINEAR and kind not in RQ and nt > 4:
        Xt[2], Xt[3] = 1e3, -1e3
        far = [2, 3]
    out = z[name + "/out"]
    return dict(kind=kind, X=np.asfortranarray(z[g + "/X"]), y=z[g + "/y"], Xt=Xt, mean=float(m[4]), logNoise=float(m[5]),
                cond=float(m[6]), dup=(int(m[7]), int(m[8])), loghyp=np.array(m[9:]), far=far, dmu=out[:, :D], dvar=out[:, D:])


def aggregate_gradients(family, mu, var, dmu, dvar, ent, coef=None, group=None, G=0, plain=False, kss_prior=None,
                        noise_prior=None, dkss_prior=None, log=None):
    """pred_tolerance.aggregate differentiated step by step, over any arithmetic (mpmath at 50 digits in the fixture's generator,
    `Prop` in the tests): per test row r the lists (dmu[r][d], dvar[r][d]) from the per-entry moments mu[e], var[e] and their
    gradients dmu[e][d], dvar[e][d].  A leaf variance the mixture clamps (sigma^2 <= 0 -> 1e-8) is a constant; groups that did
    not see the row are skipped in rBCM, whose prior term s = kss_prior[r] + noise_prior has the gradient dkss_prior[r][d]."""
    from pred_tolerance import Prop
    out_m, out_v = [], []
    for r, er in enumerate(ent):
        D = len(dmu[er[0][1]]) if er else 0
        gm, gv = [], []
        for d in range(D):
            if family == 0:
                s0 = ds0 = acc = 0
                for l, e in er:
                    s0 = s0 + float(coef[l]) * mu[e]
                    ds0 = ds0 + float(coef[l]) * dmu[e][d]
                for l, e in er:
                    v = var[e]
                    clamped = not (v.v if isinstance(v, Prop) else v) > 0
                    w = float(coef[l])
                    if not clamped:
                        acc = acc + w * dvar[e][d]
                    if not plain:
                        acc = acc + w * (2 * (mu[e] - s0) * dmu[e][d])
                gm.append(ds0)
                gv.append(acc)
                continue

            def sums(entries, bt):
                T = P = dT = dP = 0
                for l, e in entries:
                    t = bt(l) * (1 / var[e])
                    T = T + t
                    P = P + t * mu[e]
                    dT = dT - (t / var[e]) * dvar[e][d]
                    dP = dP + (t * dmu[e][d] - (t * mu[e] / var[e]) * dvar[e][d])
                return T, P, dT, dP

            if family != 3:
                T, P, dT, dP = sums(er, lambda l: float(coef[l]))
                m = P / T
                gm.append((dP - m * dT) / T)
                gv.append(0 - dT / (T * T))
                continue
            s = kss_prior[r] + noise_prior
            ds = dkss_prior[r][d]
            C, dC, mm, dmm = 1 / s, 0 - ds / (s * s), 0, 0
            for g in range(G):
                eg = [(l, e) for l, e in er if group[l] == g]
                if not eg:
                    continue
                T, P, dT, dP = sums(eg, lambda l: 1.0)
                beta = (log(s) + log(T)) * 0.5
                dbeta = (ds / s + dT / T) * 0.5
                C = C + beta * (T - 1 / s)
                dC = dC + dbeta * (T - 1 / s) + beta * (dT + ds / (s * s))
                mm = mm + beta * P
                dmm = dmm + dbeta * P + beta * dP
            m = mm / C
            gm.append((dmm - m * dC) / C)
            gv.append(0 - dC / (C * C))
        out_m.append(gm)
        out_v.append(gv)
    return out_m, out_v
