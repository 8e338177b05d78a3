"""CPU tests of the leaf-count edges (tests/many_leaves_cases.py): the longdouble reference against 50-digit evaluations from the
definitions, the tables against their description, the tables' power to fail a library that takes the wrong leaf past a chunk
edge, the tolerances restated over the leaf axis against the functions they restate, and the chunk helper on the host."""
import os
import re
import subprocess

import mpmath as mp
import numpy as np
import pytest

import kfold_dense as kd
import loo_dense
import many_leaves_cases as mc
import targets_dense as td
from pred_tolerance import alpha_tol, mll_tol, moment_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc")
CHUNK = mc.CHUNK
DEVICE_KEYS = ("mll", "alpha", "grad", "loo_mu", "loo_var", "loo_lpd", "kfold_mu", "kfold_var", "kfold_lpd", "targets_mll",
               "targets_z", "targets_loo_mu", "targets_loo_lpd", "pred_mu", "pred_var")


@pytest.fixture(scope="module", params=["A", "B"])
def tab(request):
    t = mc.table(request.param)
    ref = mc.reference(t)
    return t, ref, mc.tolerances(t, ref)


def _sample(t, count=200):
    """The small leaves next to the edges and the special ones, every fourth routed leaf, filled up to `count` with a fixed draw
    over the table."""
    first = [int(l) for l in list(t.edge_leaves) + list(t.routed[::4]) if t.n[l] <= 3]
    draw = [int(l) for l in (mc.uniform(7201, 0, 4 * count) * t.L).astype(np.int64) if t.n[l] <= 3]
    out = list(dict.fromkeys(first + draw))[:count]
    assert len(out) == count and set(first) <= set(out)
    return np.array(sorted(out), dtype=np.int64)


# ------------------------------------------------------------------------------------- (1) the chunk helper and the sources

def test_chunk_helper_on_the_host(tmp_path):
    """csrc/leaf_chunks.hpp is plain C++17: tests/leaf_chunks_check.cpp, compiled with g++, checks L = 1, 32767, 32768, 32769,
    65535, 65536, 65537, 65600 (and 0 and 10^6): an ascending partition of 0 .. L - 1, every run of at most 32,768 leaves."""
    exe = str(tmp_path / "leaf_chunks_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, os.path.join(ROOT, "tests", "leaf_chunks_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0 and "FAILED" not in run.stdout and run.stdout.rstrip().endswith("all cases passed"), run.stdout + run.stderr
    for L in (1, 32767, 32768, 32769, 65535, 65536, 65537, 65600):
        assert f"count {L}:" in run.stdout
    src = open(os.path.join(CSRC, "leaf_chunks.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()


def test_no_kernel_indexes_the_leaf_table_by_its_grid_row_alone():
    """A kernel with one grid row per leaf takes the first leaf of its run: `leaves[blockIdx.y]` appears nowhere in csrc/.  The
    header and INTEGRATION.md state the contract: the leaf count is bounded by device memory only, and `needed` covers the fit's
    arenas only."""
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cpp", ".hpp")):
            for i, line in enumerate(open(os.path.join(CSRC, name)), 1):
                assert not re.search(r"leaves\[blockIdx\.y\]", line), (name, i, line)
    for path in (os.path.join(ROOT, "include", "dsmgp_hip.h"), os.path.join(ROOT, "INTEGRATION.md")):
        text = " ".join(open(path).read().replace(" * ", " ").split())
        for phrase in ("bounded by device memory only", "covers the arenas of the fit only"):
            assert phrase in text, (path, phrase)


# ------------------------------------------------------------------------------------- (2) the tables are what the docstring says

def test_tables_are_what_the_docstring_says(tab):
    t, ref, tol = tab
    L = t.L
    assert L == mc.SIZES[t.name] and t.obs_ptr.size == L + 1 and t.obs_idx.size == t.obs_ptr[-1]
    assert (L == 33000 and L > CHUNK) if t.name == "A" else (L == 65600 and L - 2 * CHUNK == 64)
    special = set(t.big) | set(t.special.values())
    for l in range(L) if L < 40000 else list(range(0, L, 7)) + list(t.edge_leaves):
        if l not in special:
            assert t.n[l] == 1 + l % 3 and t.kid[l] == l % 3, l
    assert [t.n[l] for l in (0, CHUNK - 1, CHUNK, L - 1)] == [130, 130, 300, 130]
    assert np.all(np.diff(t.obs_ptr) == t.n)
    # ascending inside a leaf; disjoint row sets apart from the two sharing claims; every training row used
    inside = np.ones(t.obs_idx.size, dtype=bool)
    inside[t.obs_ptr[1:-1]] = False
    assert np.all(np.diff(t.obs_idx)[inside[1:]] > 0)
    owner = np.repeat(np.arange(L), t.n)
    shared = np.isin(owner, [mc.COPY_LEAF, mc.PREFIX_LEAF]) if t.name == "A" else np.zeros(owner.size, dtype=bool)
    rows = t.obs_idx[~shared]
    assert np.unique(rows).size == rows.size
    assert np.unique(t.obs_idx).size == t.N
    # a permutation: leaf l and leaf l - 32768 are not an offset of each other, and share no row
    l = np.arange(CHUNK + 5, min(L, CHUNK + 2000))
    l = l[(t.n[l] <= 3) & (t.n[l - CHUNK] <= 3)]
    assert np.all(t.obs_idx[t.obs_ptr[l]] != t.obs_idx[t.obs_ptr[l - CHUNK]])
    assert np.std(t.obs_idx[t.obs_ptr[l]] - t.obs_idx[t.obs_ptr[l - CHUNK]]) > t.N / 10
    # means, targets
    for q in (5, CHUNK + 7, L - 3):
        r = t.obs_idx[t.obs_ptr[q]:t.obs_ptr[q + 1]]
        assert abs(t.mean[q] - (np.mean(t.y[r]) + 0.01 * (q % 7))) < 1e-14
        assert np.allclose(t.Ymean[q], np.mean(t.Y[r], axis=0) + 0.01 * (q % 7), rtol=0, atol=1e-12)
    assert t.Y.shape == (t.N, 3) and np.min(t.Y[:, 2]) > 990 and np.max(np.abs(t.Y[:, :2])) < 10
    # routes: about 400 leaves of 6 rows, both sides of every edge, every test row used once
    assert 330 <= t.routed.size <= 420 and np.all(t.nt[t.routed] == mc.NT) and t.nt.sum() == mc.NT * t.routed.size == t.n_t
    for e in mc.EDGES + (L - 1,):
        for d in range(-2, 3):
            if 0 <= e + d < L:
                assert t.nt[e + d] == mc.NT, (e, d)
    assert np.array_equal(np.sort(t.route_idx), np.arange(t.n_t))
    last0 = (L - 1) // CHUNK * CHUNK
    assert np.sum(t.routed >= last0) >= 30 and np.sum(t.routed < CHUNK) >= 100
    # the special leaves
    if t.name == "A":
        c, s, p, ps, f = mc.COPY_LEAF, mc.COPY_SRC, mc.PREFIX_LEAF, mc.PREFIX_SRC, mc.FAILED
        assert (c, p, f) == (32770, 32771, 32790) and (s, ps) == (5, 32767)
        rows_of = lambda q: t.obs_idx[t.obs_ptr[q]:t.obs_ptr[q + 1]]       # noqa: E731
        assert np.array_equal(rows_of(c), rows_of(s)) and t.kid[c] == t.kid[s] and t.mean[c] != t.mean[s]
        assert t.op[c] == mc.COPY and t.src[c] == s
        assert t.n[p] == 150 and np.array_equal(rows_of(p)[:130], rows_of(ps)) and t.kid[p] == t.kid[ps]
        assert t.op[p] == mc.PREFIX and t.src[p] == ps and t.plen[p] == 130 and t.plen[p] // 128 == 1
        assert np.sum(t.op != 0) == 2
        assert np.sum(t.kid == 3) == 1 and t.kid[f] == 3 and t.n[f] == 140 and np.min(t.X[rows_of(f), 0]) >= 1e8
        assert t.nt[f - 1] == t.nt[f + 1] == t.nt[f] == mc.NT and t.n[f - 1] <= 3 and t.n[f + 1] <= 3
        assert t.large == [0, ps, CHUNK, p, L - 1]
    else:
        assert not t.special and np.all(t.op == 0) and t.large == [0, CHUNK - 1, CHUNK, L - 1] and np.all(t.kid < 3)
    assert tol["cond"].max() < 1e3
    print(f"\ntable {t.name}: L {L}, N {t.N}, routed leaves {t.routed.size}, test rows {t.n_t}, largest cond_2 {tol['cond'].max():.4g}")


# ------------------------------------------------------------------------------------- (3) the restated tolerances

def test_leaf_axis_tolerances_are_the_projects_functions(tab):
    """`tolerances` against pred_tolerance / loo_dense / kfold_dense / targets_dense called leaf by leaf on the sample."""
    t, _, _ = tab
    sel = _sample(t)
    ref = mc.reference(t, sel)
    tol = mc.tolerances(t, ref)
    f = lambda a: np.asarray(a, dtype=np.float64)       # noqa: E731
    close = lambda a, b: np.allclose(a, b, rtol=1e-9, atol=0)      # noqa: E731
    ri = {int(l): i for i, l in enumerate(ref["routed"])}
    for i, l in enumerate(sel):
        n = int(t.n[l])
        rows = ref["rows"][i, :n]
        y, cond, noise = t.y[rows], float(tol["cond"][i]), float(ref["noise"][i])
        kss = f(ref["kss"][i, :n])
        assert close(tol["mll"][i], mll_tol(f(ref["mll"][i]), cond))
        assert close(tol["alpha"][i, 0], alpha_tol(f(ref["alpha"][i, :n]), cond))
        tm, tv, _, ts = loo_dense.loo_tol(y, f(ref["loo_mu"][i, :n]), f(ref["loo_var"][i, :n]), kss, noise)
        assert close(tol["loo_mu"][i, :n], tm) and close(tol["loo_var"][i, :n], tv) and close(tol["loo_lpd"][i], ts)
        km, kv = kd.moment_tols(y, f(ref["kfold_mu"][i, :n]), f(ref["kfold_var"][i, :n]), kss, noise)
        assert close(tol["kfold_mu"][i, :n], km) and close(tol["kfold_var"][i, :n], kv)
        Z = f(ref["targets_z"][i, :n])
        assert close(tol["targets_z"][i, :n], td.z_tol(Z, cond))
        F = np.diag(np.exp(np.full(n, f(ref["half_logdet"][i]) / n)))            # (mll_tol reads sum log F_ii alone)
        assert close(tol["targets_mll"][i], td.mll_tol(Z, F, cond))
        for q in range(mc.Q):
            tm, _, _, ts = loo_dense.loo_tol(t.Y[rows, q], f(ref["targets_loo_mu"][i, :n, q]), f(ref["loo_var"][i, :n]), kss, noise)
            assert close(tol["targets_loo_mu"][i, :n, q], tm) and close(tol["targets_loo_lpd"][i, q], ts)
        if i in ri:
            j = ri[i]
            pm, pv = moment_tol(f(ref["pred_mu"][j]), f(ref["pred_var"][j]), f(ref["pred_kss"][j]), noise,
                                max(1.0, float(np.max(np.abs(y)))))
            assert close(tol["pred_mu"][j], pm) and close(tol["pred_var"][j], pv)
    # cond and |K_y|_2 against the dense float64 matrix, and k-fold's backward bound, on a few leaves
    import dense_kernels as dk
    for i in range(0, sel.size, 17):
        l, n = int(sel[i]), int(t.n[sel[i]])
        rows = ref["rows"][i, :n]
        hyp = np.array(mc.HYP[t.kid[l]])
        Ky = dk.noisy(dk.value(mc.KINDS[t.kid[l]], hyp[:-1], t.X[rows], t.X[rows]), np.exp(2.0 * hyp[-1]))
        ev = np.linalg.eigvalsh(Ky)
        assert close(tol["cond"][i], ev[-1] / ev[0])
        back = kd.lpd_tol_backward(n, ev[-1] / ev[0], f(ref["alpha"][i, :n]), ev[-1])
        for k in range(mc.KFOLDS):
            cnt = int(np.sum(ref["labels"][i] == k))
            assert close(tol["kfold_lpd"][i, k], back + kd.lpd_floor(cnt, f(ref["kfold_abs"][i, k])))


# ------------------------------------------------------------------------------------- (4) the reference is right

mp.mp.dps = 50


def _mp_kernel(kid, hyp, a, b):
    if kid == 0:
        return mp.exp(2 * hyp[1]) * mp.exp(-sum((p - q) ** 2 for p, q in zip(a, b)) / (2 * mp.exp(2 * hyp[0])))
    if kid == 1:
        return mp.exp(2 * hyp[2]) * mp.exp(-sum((p - q) ** 2 / mp.exp(2 * hyp[d]) for d, (p, q) in enumerate(zip(a, b))) / 2)
    return sum(p * q / mp.exp(2 * hyp[d]) for d, (p, q) in enumerate(zip(a, b)))


def _mp_Ky(kid, hyp, X):
    n = len(X)
    noise = mp.exp(2 * hyp[-1])
    return mp.matrix(n, n) + mp.matrix([[_mp_kernel(kid, hyp, X[i], X[j]) + ((noise + mp.mpf(1e-8)) if i == j else 0) for j in range(n)]
                                        for i in range(n)])


def _mp_mll(kid, hyp, X, yc):
    Ky = _mp_Ky(kid, hyp, X)
    a = mp.lu_solve(Ky, yc)
    return -((yc.T * a)[0] + mp.log(mp.det(Ky)) + len(X) * mp.log(2 * mp.pi)) / 2


def _mp_density(y, mu, S):
    """log N(y | mu, S) of a joint Gaussian from the definition."""
    r = y - mu
    return -((r.T * mp.lu_solve(S, r))[0] + mp.log(mp.det(S)) + len(y) * mp.log(2 * mp.pi)) / 2


def _mp_heldout(kid, hyp, X, y, mean, F):
    """The GP refitted without the rows F (same mean, hyper-parameters and jitter) predicts them jointly: (mu, Sigma)."""
    n = len(X)
    rest = [i for i in range(n) if i not in F]
    Ky = _mp_Ky(kid, hyp, X)
    mu = mp.matrix([mean] * len(F))
    S = mp.matrix([[Ky[i, j] for j in F] for i in F])
    if rest:
        Krr = mp.matrix([[Ky[i, j] for j in rest] for i in rest])
        Kfr = mp.matrix([[Ky[i, j] for j in rest] for i in F])
        mu = mu + Kfr * mp.lu_solve(Krr, mp.matrix([y[i] - mean for i in rest]))
        S = S - Kfr * (mp.inverse(Krr) * Kfr.T)
    return mu, S


def _mp_leaf(t, l):
    n, kid = int(t.n[l]), int(t.kid[l])
    rows = t.obs_idx[t.obs_ptr[l]:t.obs_ptr[l + 1]]
    hyp = [mp.mpf(float(v)) for v in mc.HYP[kid]]
    X = [[mp.mpf(float(v)) for v in t.X[r]] for r in rows]
    out = {}

    def column(yv, mean):
        y = mp.matrix([mp.mpf(float(v)) for v in yv])
        mean = mp.mpf(float(mean))
        yc = y - mp.matrix([mean] * n)
        loo = [_mp_heldout(kid, hyp, X, y, mean, [i]) for i in range(n)]
        lmu = [m_[0] for m_, _ in loo]
        lvar = [S[0, 0] for _, S in loo]
        lpd = sum(_mp_density(mp.matrix([y[i]]), mp.matrix([lmu[i]]), mp.matrix([[lvar[i]]])) for i in range(n))
        return y, mean, yc, _mp_mll(kid, hyp, X, yc), lmu, lvar, lpd, mp.lu_solve(mp.cholesky(_mp_Ky(kid, hyp, X)), yc)

    y, mean, yc, out["mll"], out["loo_mu"], out["loo_var"], out["loo_lpd"], _ = column(t.y[rows], t.mean[l])
    Ky = _mp_Ky(kid, hyp, X)
    alpha = mp.lu_solve(Ky, yc)
    out["alpha"] = list(alpha)
    # the gradient: the derivative of the log marginal itself, slot by slot, in the convention of dsmgp_gradients
    g = []
    for s in range(len(hyp)):
        fs = lambda v, s=s: _mp_mll(kid, hyp[:s] + [v] + hyp[s + 1:], X, yc)       # noqa: E731
        d = mp.diff(fs, hyp[s])
        g.append(d * mp.exp(hyp[1]) if kid == 0 and s < 2 else d)
    out["grad"] = g + [mp.mpf(0)] * (mc.STRIDE - len(g))
    kmu, kvar, klpd = [mp.nan] * n, [mp.nan] * n, []
    for k in range(mc.KFOLDS):
        F = [i for i in range(n) if rows[i] % mc.KFOLDS == k]
        if not F:
            klpd.append(mp.mpf(0))
            continue
        mu, S = _mp_heldout(kid, hyp, X, y, mean, F)
        klpd.append(_mp_density(mp.matrix([y[i] for i in F]), mu, S))
        for j, i in enumerate(F):
            kmu[i], kvar[i] = mu[j], S[j, j]
    out["kfold_mu"], out["kfold_var"], out["kfold_lpd"] = kmu, kvar, klpd
    cols = [column(t.Y[rows, q], t.Ymean[l, q]) for q in range(mc.Q)]
    out["targets_mll"] = [c[3] for c in cols]
    out["targets_loo_mu"] = [[c[4][i] for c in cols] for i in range(n)]
    out["targets_loo_lpd"] = [c[6] for c in cols]
    out["targets_z"] = [[c[7][i] for c in cols] for i in range(n)]
    if t.nt[l]:
        noise = mp.exp(2 * hyp[-1])
        pm, pv = [], []
        for e in range(int(t.route_ptr[l]), int(t.route_ptr[l + 1])):
            xt = [mp.mpf(float(v)) for v in t.Xt[t.route_idx[e]]]
            kt = mp.matrix([_mp_kernel(kid, hyp, xt, X[i]) for i in range(n)])
            pm.append(mean + (kt.T * alpha)[0])
            pv.append(_mp_kernel(kid, hyp, xt, xt) - (kt.T * mp.lu_solve(Ky, kt))[0] + noise)
        out["pred_mu"], out["pred_var"] = pm, pv
    return out


def test_reference_against_50_digit_definitions(tab):
    """200 leaves of each table, every small leaf next to an edge among them: every quantity of the longdouble reference within
    1/20 of its device tolerance of a 50-digit evaluation from the definitions (log marginal and solve by LU at 50 digits, the
    gradient as the derivative of the log marginal, LOO and k-fold by refitting without the held-out rows)."""
    t, _, _ = tab
    sel = _sample(t)
    ref = mc.reference(t, sel)
    tol = mc.tolerances(t, ref)
    ri = {int(i): j for j, i in enumerate(ref["routed"])}
    worst = {}

    def see(key, got, want, tl):
        r = float(abs(mp.mpf(float(got)) + mp.mpf(float(got - np.longdouble(float(got)))) - want) / mp.mpf(float(tl)))
        worst[key] = max(worst.get(key, 0.0), r)

    for i, l in enumerate(sel):
        n = int(t.n[l])
        m = _mp_leaf(t, int(l))
        see("mll", ref["mll"][i], m["mll"], tol["mll"][i])
        see("loo_lpd", ref["loo_lpd"][i], m["loo_lpd"], tol["loo_lpd"][i])
        for s in range(mc.STRIDE):
            see("grad", ref["grad"][i, s], m["grad"][s], tol["grad"][i, s])
        for r in range(n):
            for key in ("alpha", "loo_mu", "loo_var"):
                see(key, ref[key][i, r], m[key][r], tol[key][i, r])
            for key in ("kfold_mu", "kfold_var"):
                assert mp.isnan(m[key][r]) == bool(np.isnan(ref[key][i, r]))
                if not mp.isnan(m[key][r]):
                    see(key, ref[key][i, r], m[key][r], tol[key][i, r])
            for q in range(mc.Q):
                see("targets_loo_mu", ref["targets_loo_mu"][i, r, q], m["targets_loo_mu"][r][q], tol["targets_loo_mu"][i, r, q])
                see("targets_z", ref["targets_z"][i, r, q], m["targets_z"][r][q], tol["targets_z"][i, r, q])
        assert np.all(np.isnan(np.asarray(ref["alpha"][i, n:], dtype=np.float64)))
        for k in range(mc.KFOLDS):
            see("kfold_lpd", ref["kfold_lpd"][i, k], m["kfold_lpd"][k], tol["kfold_lpd"][i, k])
        for q in range(mc.Q):
            see("targets_mll", ref["targets_mll"][i, q], m["targets_mll"][q], tol["targets_mll"][i, q])
            see("targets_loo_lpd", ref["targets_loo_lpd"][i, q], m["targets_loo_lpd"][q], tol["targets_loo_lpd"][i, q])
        if i in ri:
            for j in range(mc.NT):
                see("pred_mu", ref["pred_mu"][ri[i], j], m["pred_mu"][j], tol["pred_mu"][ri[i], j])
                see("pred_var", ref["pred_var"][ri[i], j], m["pred_var"][j], tol["pred_var"][ri[i], j])
    print(f"\ntable {t.name}: {sel.size} leaves ({len(ri)} routed), worst |reference - 50 digits| / device tolerance:")
    for k, v in sorted(worst.items()):
        print(f"    {k:16s} {v:.3g}")
    assert set(worst) == set(DEVICE_KEYS) and len(ri) >= 60
    assert max(worst.values()) <= 1.0 / 20.0, worst


# ------------------------------------------------------------------------------------- (5) the tables can fail a wrong library

# what a wrong first leaf in each gather must move, on EVERY small leaf at or past the edge (a variance of a one-row leaf of a
# stationary kernel does not see its inputs: the variances are reported, not required, under the training-row wraps)
REQUIRED = {"train": ("mll", "alpha", "grad", "loo_mu", "loo_lpd", "kfold_lpd", "pred_mu", "pred_var"),
            "test": ("pred_mu", "pred_var"),
            "target": ("targets_mll", "targets_z", "targets_loo_mu", "targets_loo_lpd")}
# a held-out mean of a one-row leaf is its prior mean, whatever its row: required from two rows on
FROM_TWO_ROWS = ("loo_mu", "targets_loo_mu")
# (a fold that holds every row of a leaf is predicted by the prior mean too: kfold_mu is reported)
# (the target columns keep their own rows under a wrapped gather_leaf_kernel: their log marginals move through the factor alone,
#  and the factor of a one-row leaf of a stationary kernel is a constant: reported)
REPORTED = {"train": ("kfold_mu", "loo_var", "kfold_var", "targets_mll"), "test": (), "target": ()}


def _leaf_ratio(key, a, b, tl):
    """Per leaf the largest |a - b| / tol over its entries (NaN on both sides: no entry)."""
    d = np.abs(a - b).astype(np.float64) / tl
    d = np.where(np.isnan(np.asarray(a, dtype=np.float64)) & np.isnan(np.asarray(b, dtype=np.float64)), 0.0, d)
    return d.reshape(d.shape[0], -1).max(axis=1)


@pytest.mark.parametrize("which", ["train", "test", "target"])
def test_wrapped_leaf_indices_miss_the_tolerance(tab, which):
    t, ref, tol = tab
    sel, R = ref["leaves"], ref["routed"]
    print()
    for name, (wrap, edge) in mc.WRAPS.items():
        wr = mc.reference(t, **{which + "_wrap": wrap})
        past, past_r = sel >= edge, sel[R] >= edge
        for key in DEVICE_KEYS:
            a, b = ref[key], wr[key]
            below = ~(past_r if key.startswith("pred_") else past)
            assert np.array_equal(a[below], b[below], equal_nan=True), (name, key)       # to the last of the 64 bits
        if not past.any():
            print(f"table {t.name}, {which} rows of leaf {name}: no leaf at or past {edge}, every leaf untouched")
            assert t.L <= edge
            continue
        line = []
        for key in REQUIRED[which] + REPORTED[which]:
            p = past_r if key.startswith("pred_") else (past & (ref["n"] >= 2) if key in FROM_TWO_ROWS else past)
            if which == "test" and key == "pred_mu":
                # a one-row leaf with l % 7 == 0 has its y as its mean: alpha = 0 and the mean of every test row is the leaf's
                # mean (its variance is required like every other leaf's)
                p = p & ~((ref["n"][R] == 1) & (sel[R] % 7 == 0))
            assert p.sum() >= 20, (name, key)
            r = _leaf_ratio(key, ref[key][p], wr[key][p], tol[key][p])
            line.append(f"{key} {r.min():.3g}" + ("" if key in REQUIRED[which] else f" ({int(np.sum(r > 1))}/{r.size} miss)"))
            if key in REQUIRED[which]:
                assert r.min() > 1.0, (t.name, which, name, key, int((sel[R] if key.startswith("pred_") else sel)[p][np.argmin(r)]), r.min())
        print(f"table {t.name}, {which} rows of leaf {name}: {int(past.sum())} leaves past the edge ({int(past_r.sum())} routed), "
              f"smallest miss / tolerance: " + ", ".join(line))
