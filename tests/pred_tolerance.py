"""The aggregation formula of predict and the tolerances of tests/golden/gp_pred.npz, in one place.

`aggregate` is what agg_partial_kernel and agg_finish_kernel evaluate (deepstructuredmixtures_amd/csrc/kernels_agg.hpp, the
comment at its head and the agg_* rule functions), written once over any arithmetic: tests/golden/make_pred_golden.py runs it at 50 digits (mpmath),
the tests run it on `Prop` values to carry the per-entry tolerances through the same operations.  Every tolerance the
prediction tests use is a function below; each docstring says where it comes from."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
RTOL = 1e-8          # north star: predictive moments within 1e-8 relative
ATOL = 1e-11         # the absolute term of the gp_edge test, per unit of the quantity's own scale
LOG2PI = 1.8378770664093454835606594728112


class Prop:
    """A float64 value with a first-order bound on its error, carried through + - * / log sqrt abs:
    |d(a + b)| <= |da| + |db|, |d(ab)| <= |a||db| + |b||da|, |d(a / b)| <= |da| / |b| + |a||db| / b^2, |d log a| <= |da| / |a|,
    |d sqrt a| <= |da| / (2 sqrt a)."""

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Prop) else Prop(x)

    def __add__(self, o):
        o = Prop.of(o)
        return Prop(self.v + o.v, self.e + o.e)

    __radd__ = __add__

    def __sub__(self, o):
        o = Prop.of(o)
        return Prop(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return Prop.of(o) - self

    def __mul__(self, o):
        o = Prop.of(o)
        return Prop(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Prop.of(o)
        return Prop(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def __rtruediv__(self, o):
        return Prop.of(o) / self

    def log(self):
        return Prop(np.log(self.v), self.e / np.abs(self.v))

    def sqrt(self):
        s = np.sqrt(self.v)
        return Prop(s, self.e / (2 * s))

    def abs(self):
        return Prop(np.abs(self.v), self.e)

    def sum(self):
        return Prop(np.sum(self.v), np.sum(self.e))

    def mean(self):
        return Prop(np.mean(self.v), np.mean(self.e))


def row_entries(route_ptr, route_idx, n_t):
    """Per test row its (leaf, entry) pairs in ascending entry order = leaf order, the order agg_partial_kernel adds them."""
    ent = [[] for _ in range(n_t)]
    for l in range(len(route_ptr) - 1):
        for e in range(int(route_ptr[l]), int(route_ptr[l + 1])):
            ent[int(route_idx[e])].append((l, e))
    return ent


def aggregate(family, mu, var, ent, coef=None, group=None, G=0, plain=False, kss_prior=None, noise_prior=None, log=None):
    """(mu, var) per test row of one family, from the per-entry moments (lists of scalars of one arithmetic), `ent` =
    row_entries(...), `log` = that arithmetic's logarithm.  family 0 mixture: S0 = sum W mu, S1 = sum W mu^2, S2 = sum W
    sigma^2 (sigma^2 <= 0 -> 1e-8), mu = S0, var = S2 (plain) or S2 + (S1 - S0^2); 1 PoE / 2 gPoE: t = beta / sigma^2,
    mu = sum t mu / sum t, var = 1 / sum t; 3 rBCM: per group g the PoE sums (T_g mu_g, T_g), s = k(x*, x*) + noise of the
    prior kernel, C = 1/s + sum_g (beta_g T_g - beta_g / s) and m = sum_g mu_g beta_g T_g with beta_g = (log s - log(1/T_g)) / 2
    over the groups that saw the row, mu = m / C, var = 1 / C (src/common.jl:137,145-149,198-241,275-302)."""
    out_mu, out_var = [], []
    for r, er in enumerate(ent):
        if family == 0:
            s0 = s1 = s2 = 0
            for l, e in er:
                w, m, v = float(coef[l]), mu[e], var[e]
                if not (v.v if isinstance(v, Prop) else v) > 0:
                    v = 1e-8
                s0 = s0 + w * m
                s1 = s1 + w * (m * m)
                s2 = s2 + w * v
            out_mu.append(s0)
            out_var.append(s2 if plain else s2 + (s1 - s0 * s0))
        elif family == 3:
            S = [[0, 0] for _ in range(G)]
            for l, e in er:
                t = 1 / var[e]
                S[group[l]][0] = S[group[l]][0] + t * mu[e]
                S[group[l]][1] = S[group[l]][1] + t
            s = kss_prior[r] + noise_prior
            C, m = 1 / s, 0
            for g in range(G):
                if not any(group[l] == g for l, _ in er):
                    continue                               # no leaf of this group saw the row
                T = S[g][1]
                beta = (log(s) - log(1 / T)) * 0.5
                C = C + beta * T - beta / s
                m = m + (S[g][0] / T) * (beta * T)
            out_mu.append(m / C)
            out_var.append(1 / C)
        else:
            s0 = s1 = 0
            for l, e in er:
                bt = float(coef[l]) * (1 / var[e])
                s0 = s0 + bt * mu[e]
                s1 = s1 + bt
            out_mu.append(s0 / s1)
            out_var.append(1 / s1)
    return out_mu, out_var


def moment_tol(mu, var, kss, noise, yscale):
    """Per (leaf, row) entry: the north star RTOL relative, plus ATOL times the quantity's own scale -- the target's magnitude
    max(1, max|y|) for mu, the prior variance max(1, k(x*, x*) + noise) for sigma^2 (near a training input sigma^2 is the
    small difference of k** + noise and |L^-1 k*|^2, both of that size)."""
    mu, var, kss = (np.asarray(a, dtype=np.float64) for a in (mu, var, kss))
    return RTOL * np.abs(mu) + ATOL * yscale, RTOL * np.abs(var) + ATOL * np.maximum(1.0, kss + noise)


def mll_tol(mll, cond):
    """Log-marginal of one leaf: 64 cond_2(K_y) eps relative to max(1, |mll|), floored at 1e-13 (as the gradient fixture)."""
    return np.maximum(1e-13, 64.0 * np.asarray(cond) * EPS * np.maximum(1.0, np.abs(mll)))


def alpha_tol(alpha, cond):
    """alpha = K_y^-1 (y - m) of one leaf: the forward error of a backward-stable solve, 64 cond_2(K_y) eps max|alpha|."""
    return max(1e-13, 64.0 * float(cond) * EPS * float(np.max(np.abs(alpha))))


def agg_tol(family, mu, var, tol_mu, tol_var, ent, S1=None, **kw):
    """(tol mu, tol var) per test row of an aggregate: the per-entry tolerances carried through the same formula (Prop), plus
    16 eps |value| for the device's own rounding of a few terms per row.  The mixture variance S2 + (S1 - S0^2) is the
    exception: its dependence on the means cancels to first order where they agree (d var / d mu_l = 2 W_l (mu_l - S0)), which
    term-by-term propagation cannot see, so it gets the sigma^2 part carried through, the north-star RTOL |var| for the means,
    and on top the floor of that formula in float64, 4 eps S1 -- S1 = sum W mu^2 and S0^2 are each rounded at magnitude S1,
    and the sums that form them carry that much again (the reference's own arithmetic, src/common.jl:299-300; with mu ~ 1000
    and a variance ~ 0.01 it is all the formula can give: DESIGN.md section 3)."""
    pm = [Prop(m, t) for m, t in zip(mu, tol_mu)]
    pv = [Prop(v, t) for v, t in zip(var, tol_var)]
    if family == 3:
        kw = dict(kw, kss_prior=[Prop(v) for v in kw["kss_prior"]])
    am, av = aggregate(family, pm, pv, ent, log=Prop.log, **kw)
    m = np.array([Prop.of(a).v for a in am])
    v = np.array([Prop.of(a).v for a in av])
    tm = np.array([Prop.of(a).e for a in am]) + 16 * EPS * np.abs(m)
    tv = np.array([Prop.of(a).e for a in av]) + 16 * EPS * np.abs(v)
    if family == 0 and not kw.get("plain", False):
        _, av = aggregate(family, [Prop(m_) for m_ in mu], pv, ent, log=Prop.log, **kw)
        tv = np.array([Prop.of(a).e for a in av]) + (RTOL + 16 * EPS) * np.abs(v) + 4 * EPS * np.asarray(S1)
    return tm, tv


def score_tol(y, mu, var, tol_mu, tol_var):
    """The five scores (src/scorefunctions.jl:6-16) with the aggregated moments' tolerances carried through them, plus the
    rounding of the device's sums: 256-row block trees added in block order, (8 + n_blocks + 4) eps times the mean of |term|."""
    n = len(y)
    d = Prop(np.asarray(y, dtype=np.float64)) - Prop(mu, tol_mu)
    v = Prop(var, tol_var)
    se = d * d
    ae = d.abs()
    mse, mae = se.mean(), ae.mean()
    sse = (((se - mse) * (se - mse)).sum() / (n - 1)).sqrt() / math.sqrt(n)
    sae = (((ae - mae) * (ae - mae)).sum() / (n - 1)).sqrt() / math.sqrt(n)
    terms = (se / v + LOG2PI) * 0.5 + v.sqrt().log()
    nlpd = terms.mean()
    c = (8 + math.ceil(n / 256) + 4) * EPS
    rnd = [c * np.mean(np.abs(se.v)), c * np.mean(np.abs(se.v)), c * np.mean(np.abs(ae.v)), c * np.mean(np.abs(ae.v)),
           c * np.mean(np.abs(terms.v))]
    return np.array([float(s.e) + r for s, r in zip((mse, sse, mae, sae, nlpd), rnd)])
