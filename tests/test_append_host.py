"""CPU tests of appending training rows to a fitted model: the C ABI's declarations and exports, and the host side of
model.add_data -- routing of the new rows, grown lists, default means, the follow-up fit, refusals and the out-of-memory fallback --
over a stand-in context that refits the grown table on the CPU oracle (tests/append_context.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import append_tables as at
import deepstructuredmixtures_amd as dsm
from append_context import AppendOracleContext, grow_by_hand
from deepstructuredmixtures_amd import hipabi
from oracle import gp as ogp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsmgp_append_rows": ("int", ["dsmgp_ctx*", "double*", "double*", "int64_t", "int32_t", "int64_t*", "int64_t*", "double*",
                                     "double*", "int32_t*", "double*"]),
       "dsmgp_append_stats": ("int", ["dsmgp_ctx*", "int64_t*"])}
FAMILIES = ["dsmgp", "poe", "gpoe", "rbcm", "gp"]


def _header_prototypes(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b((?:const\s+)?(?:int64_t|int|char|void|double)\s*\**)\s*(dsmgp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        def norm(t):
            mm = re.match(r"\s*([A-Za-z_]\w*)\s*((?:\*\s*)*)", re.sub(r"\bconst\b", " ", t))
            return mm.group(1) + "*" * mm.group(2).count("*")
        args = m.group(3)
        protos[m.group(2)] = (norm(m.group(1)), [norm(a) for a in args.split(",")] if args.strip() not in ("", "void") else [])
    return protos


def test_header_declares_and_library_exports_the_two_functions():
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    protos = _header_prototypes(header)
    for name, sig in NEW.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert name in hipabi.SIGNATURES and len(hipabi.SIGNATURES[name][1]) == len(sig[1])
    # the header's prototype count grew by exactly these two: the header declares what the binding lists, and without the two
    # both are what they were
    assert set(protos) == set(hipabi.SIGNATURES)
    assert len(protos) - 2 == len([n for n in hipabi.SIGNATURES if n not in NEW])
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
    assert {s for s in exported if "append" in s.lower() and not s.startswith("_Z")} == set(NEW)      # (_Z...: the kernels' host stubs)
    assert re.search(r"#define\s+DSMGP_N_APPEND_STATS\s+6\b", header)
    assert len(hipabi.Context.APPEND_STAT_NAMES) == 6
    for phrase in ("PEAK MEMORY IS THE OLD FACTORS PLUS THE NEW ONES", "IN PLACE", "RELOCATE", "DSMGP_E_NOMEM"):
        assert phrase in header, phrase


def test_julia_ccall_sites_match_the_header():
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    for name, (_, args) in NEW.items():
        m = re.search(r"ccall\(sym\(:" + name + r"\),\s*Cint,\s*\(([^)]*)\)", src)
        assert m, name
        assert len([t for t in m.group(1).split(",") if t.strip()]) == len(args), name
    assert "function append_rows!(s::Session" in src and "function append_stats(s::Session)" in src
    export = re.search(r"(?m)^export ([^\n]*)", src).group(1)
    assert {"append_rows!", "append_stats"} <= {t.strip() for t in export.split(",")}


# ------------------------------------------------------------------------------------- add_data over the stand-in context

def _problem(n, seed, m=9):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, 2))
    y = np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]) + 3.0 + 0.1 * rng.standard_normal(n)
    xn = rng.uniform(size=(m, 2)) * 0.98 + 0.01
    yn = np.sin(3.0 * xn[:, 0]) * np.cos(2.0 * xn[:, 1]) + 3.5 + 0.1 * rng.standard_normal(m)
    xt = rng.uniform(size=(20, 2)) * 0.98 + 0.01
    return X, y, xn, yn, xt


def _build(family, X, y, mean=None):
    kw = dict(M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.2), ctx=AppendOracleContext(), seed=2)
    if family == "dsmgp":
        return dsm.buildDSMGP(X, y, 2, 4, meanFun=mean, **kw)
    if family in ("poe", "gpoe"):
        return dsm.buildPoE(X, y, 4, meanFun=mean, generalized=family == "gpoe", **kw)
    if family == "rbcm":
        return dsm.buildBCM(X, y, 4, meanFun=mean, **kw)
    g = dsm.GaussianProcess(X[:80], y[:80], mean=mean, kernel=kw["kernel"], logNoise=kw["logNoise"], ctx=kw["ctx"])
    dsm.fit(g)
    return g


@pytest.mark.parametrize("family", FAMILIES)
def test_add_data_equals_the_hand_grown_tree_fitted_from_scratch(family):
    X, y, xn, yn, xt = _problem(300, 33)
    mean = dsm.ConstMean(0.2) if family in ("poe", "gpoe") else None
    m, h = _build(family, X, y, mean), _build(family, X, y, mean)
    if family == "gp":
        X, y = X[:80], y[:80]
    tm = m.model if family == "gp" else m
    n_before = [lf.nobs for lf in tm.leaves]
    sec = dsm.add_data(m, xn, yn)
    assert isinstance(sec, float) and sec.fallback is False and sec.stats["bytes_relocated"] == 0
    grow_by_hand(family, h, xn, yn)
    th = h.model if family == "gp" else h
    assert tm.x.shape == (len(y) + len(yn), 2) and np.array_equal(tm.x, th.x) and np.array_equal(tm.y, th.y)
    grew = 0
    for a, b, n0 in zip(tm.leaves, th.leaves, n_before):
        assert np.array_equal(a.obs, b.obs) and a.nobs == b.nobs == a.obs.size and np.all(np.diff(a.obs) > 0)
        assert a.mean.m == b.mean.m
        grew += a.nobs - n0
    assert grew >= len(yn)                                  # every new row reached a leaf (sum nodes: several)
    if family == "dsmgp":
        assert grew > len(yn)
        dsm.update(m), dsm.update(h)
    if tm.D is not None:
        assert np.array_equal(np.asarray(tm.D.todense() if hasattr(tm.D, "todense") else tm.D),
                              np.asarray(th.D.todense() if hasattr(th.D, "todense") else th.D))
    assert np.allclose(tm.leaf_mll, th.leaf_mll, rtol=1e-12, atol=0) and np.array_equal(tm.leaf_info, th.leaf_info)
    assert np.isclose(dsm.mll(m), dsm.mll(h), rtol=1e-12, atol=0)
    if family == "gp":
        (mu, var), (mo, vo) = dsm.prediction(m, xt), dsm.prediction(h, xt)
    else:
        (mu, var), (mo, vo) = dsm.predict(m, xt), dsm.predict(h, xt)
    assert np.allclose(mu, mo, rtol=1e-12, atol=1e-13) and np.allclose(var, vo, rtol=1e-12, atol=1e-13)


def test_default_means_follow_the_grown_lists_and_a_user_mean_does_not_move():
    X, y, xn, yn, _ = _problem(300, 7)
    m = _build("dsmgp", X, y)
    before = [lf.mean.m for lf in m.leaves]
    dsm.add_data(m, xn, yn)
    moved = 0
    for lf, b in zip(m.leaves, before):
        assert lf.mean.default and lf.mean.m == float(np.mean(m.y[lf.obs]))
        moved += lf.mean.m != b
    assert moved > 0
    assert m.ctx.mean == [lf.mean.m for lf in m.leaves]         # what the device was given
    user = dsm.ConstMean(0.25)
    u = _build("dsmgp", X, y, user)
    dsm.add_data(u, xn, yn)
    assert all(lf.mean is user and lf.mean.m == 0.25 and not lf.mean.default for lf in u.leaves)
    assert u.ctx.mean == [0.25] * u.L


def test_the_next_fit_uploads_a_leaf_table_but_no_training_data():
    X, y, xn, yn, _ = _problem(300, 11)
    m = _build("dsmgp", X, y)
    assert m.ctx.calls.count("set_train") == 1
    del m.ctx.calls[:]
    dsm.add_data(m, xn, yn)
    assert m.ctx.calls == ["append_rows"]
    assert m.ctx.X.shape[0] == len(y) + len(yn)
    mll_appended = m.leaf_mll.copy()
    dsm.fit(m, 0.05)
    assert m.ctx.calls == ["append_rows", "set_leaves", "fit"]      # the leaf table again (new sharing decisions), not the data
    assert np.allclose(m.leaf_mll, mll_appended, rtol=1e-12, atol=0)
    dsm.fit(m, 0.05)
    assert m.ctx.calls == ["append_rows", "set_leaves", "fit", "fit"]


def test_refusals():
    X, y, xn, yn, xt = _problem(300, 13)
    m = _build("dsmgp", X, y)
    state = (m.x.copy(), m.y.copy(), [lf.obs.copy() for lf in m.leaves], [lf.mean.m for lf in m.leaves], m.leaf_mll.copy())
    calls = list(m.ctx.calls)
    bad = xn.copy()
    bad[3, 1] = np.nan                  # beyond every threshold of a split node
    with pytest.raises(hipabi.DsmgpDomainError):
        dsm.add_data(m, bad, yn)
    with pytest.raises(ValueError):
        dsm.add_data(m, xn, yn[:-1])
    with pytest.raises(ValueError):
        dsm.add_data(m, xn[:, :1], yn)
    assert m.ctx.calls == calls
    assert np.array_equal(m.x, state[0]) and np.array_equal(m.y, state[1]) and np.array_equal(m.leaf_mll, state[4])
    assert all(np.array_equal(lf.obs, o) and lf.mean.m == mu for lf, o, mu in zip(m.leaves, state[2], state[3]))
    # never fitted
    fresh = dsm.buildDSMGP(X, y, 2, 4, M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.2), ctx=AppendOracleContext(),
                           seed=2, fit_now=False)
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.add_data(fresh, xn, yn)
    assert e.value.code == hipabi.E_STATE and fresh.ctx.calls == []
    # sharded
    m.shard = type("S", (), {"world": 2, "local": m.shard.local})()
    with pytest.raises(NotImplementedError):
        dsm.add_data(m, xn, yn)
    # a context without the method
    from oracle_context import OracleContext
    plain = dsm.buildDSMGP(X, y, 2, 4, M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.2), ctx=OracleContext(), seed=2)
    with pytest.raises(NotImplementedError):
        dsm.add_data(plain, xn, yn)
    assert not hasattr(hipabi.MultiContext, "append_rows") and not hasattr(hipabi.StreamingContext, "append_rows")


def test_out_of_memory_falls_back_to_a_fit_of_the_grown_table():
    X, y, xn, yn, xt = _problem(300, 17)
    m, h = _build("dsmgp", X, y), _build("dsmgp", X, y)
    m.ctx.nomem_next_append = True
    del m.ctx.calls[:]
    sec = dsm.add_data(m, xn, yn)
    assert sec.fallback is True and sec.stats is None
    assert m.ctx.calls == ["append_rows", "set_train", "set_leaves", "fit"]
    grow_by_hand("dsmgp", h, xn, yn)
    assert np.allclose(m.leaf_mll, h.leaf_mll, rtol=1e-12, atol=0)
    assert all(np.array_equal(a.obs, b.obs) and a.mean.m == b.mean.m for a, b in zip(m.leaves, h.leaves))
    mu, var = dsm.predict(m, xt)
    mo, vo = dsm.predict(h, xt)
    assert np.allclose(mu, mo, rtol=1e-12, atol=1e-13) and np.allclose(var, vo, rtol=1e-12, atol=1e-13)
    # any other device error is not swallowed
    m.ctx.gps = []
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.add_data(m, xn, yn)
    assert e.value.code == hipabi.E_STATE


def test_the_failed_leaf_of_the_gpu_suite_fails_in_the_oracle_too():
    """The leaf tests/test_append_gpu.py uses as its failed owner -- a duplicated training row under a linear kernel of size 2^54,
    noise and jitter absorbed by rounding -- is not positive definite for oracle/gp.py either, before and after the rows are
    added, at the same leading minor (order 4: row 3 repeats row 0); the other leaves of that table are.
    This is the check on the CPU that has to come before the GPU test: it runs the test's own table through the oracle and
    touches no code of the feature, so -- unlike every other test of the feature -- it passes without it too."""
    X, y, Xn, yn, lists, adds, kid, mean = at.failed_owner_table()
    Xg, yg = np.vstack([X, Xn]), np.concatenate([y, yn])
    for l in range(len(lists)):
        kind, hyp = at.FAILED_HYP[kid[l]]
        k = ogp.make_kernel(kind, hyp[:-1])
        rows = np.concatenate([lists[l], X.shape[0] + adds[l]])
        old = ogp.GaussianProcess(X[lists[l]], y[lists[l]], mean[l], k, hyp[-1], True)
        new = ogp.GaussianProcess(Xg[rows], yg[rows], mean[l], k, hyp[-1], True)
        for g in (old, new):
            try:
                g.update_cholesky()
            except np.linalg.LinAlgError:        # potrf's info is kept; the solve for alpha then meets the zero pivot
                assert l == 0
        assert (old.info, new.info) == ((4, 4) if l == 0 else (0, 0)), (l, old.info, new.info)
        assert len(rows) <= 512          # no block step with K >= 512: no update tile is ever cut along K
