"""CPU tests of keeping the resident test set across appended rows (dsmgp_add_rows_keep_test): the C ABI's declarations and
exports, the Julia call sites, and the host side of model.add_data(..., keep_test=True) over a stand-in context that refits the
grown table on the CPU oracle and keeps its test set, as the device does (tests/append_context.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from append_context import AppendOracleContext, grow_by_hand
from deepstructuredmixtures_amd import hipabi
from test_append_host import FAMILIES, _header_prototypes, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APPEND_ARGS = ["dsmgp_ctx*", "double*", "double*", "int64_t", "int32_t", "int64_t*", "int64_t*", "double*", "double*", "int32_t*", "double*"]
NEW = {"dsmgp_add_rows_keep_test": ("int", APPEND_ARGS),
       "dsmgp_resume_stats": ("int", ["dsmgp_ctx*", "int64_t*"]),
       "dsmgp_download_vt": ("int", ["dsmgp_ctx*", "int32_t", "double*", "int64_t"])}


def test_header_declares_and_library_exports_the_three_functions():
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    protos = _header_prototypes(header)
    for name, sig in NEW.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert name in hipabi.SIGNATURES and len(hipabi.SIGNATURES[name][1]) == len(sig[1])
        assert re.search(r"(?m)^int " + name + r"\(", header), name
        assert not any(w in name for w in ("append", "target", "loo_columns")), name
    assert protos["dsmgp_add_rows_keep_test"] == protos["dsmgp_append_rows"]          # the argument list of dsmgp_append_rows
    assert set(protos) == set(hipabi.SIGNATURES)
    assert re.search(r"#define\s+DSMGP_N_RESUME_STATS\s+6\b", header) and len(hipabi.Context.RESUME_STAT_NAMES) == 6
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
    assert {s for s in exported if "append" in s.lower() and not s.startswith("_Z")} == {"dsmgp_append_rows", "dsmgp_append_stats"}


def test_julia_ccall_sites_match_the_header():
    src = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    for name, (_, args) in NEW.items():
        m = re.search(r"ccall\(sym\(:" + name + r"\),\s*Cint,\s*\(([^)]*)\)", src)
        assert m, name
        assert len([t for t in m.group(1).split(",") if t.strip()]) == len(args), name
    assert "keep_test::Bool=false" in src and "function resume_stats(s::Session)" in src and "function download_vt(s::Session" in src
    assert "function append_rows!(s::Session" in src and "ccall(sym(:dsmgp_append_rows)" in src
    export = re.search(r"(?m)^export ([^\n]*)", src).group(1)
    assert {"append_rows!", "resume_stats", "download_vt"} <= {t.strip() for t in export.split(",")}


# ------------------------------------------------------------------------------------- add_data over the stand-in context

class KeepingContext(AppendOracleContext):
    """The stand-in with the keyword: its test set (plain host arrays) survives the call, like the device's."""

    def set_test(self, Xt, route_ptr, route_idx):
        self.calls.append("set_test")
        super().set_test(Xt, route_ptr, route_idx)

    def predict_run(self):
        self.calls.append("predict_run")
        return super().predict_run()

    def append_rows(self, X_new, y_new, add_ptr, add_idx, mean=None, keep_test=False):
        out = super().append_rows(X_new, y_new, add_ptr, add_idx, mean)
        self.calls[-1] = "append_rows keep_test" if keep_test else "append_rows"
        self.kept = bool(keep_test) and hasattr(self, "Xt")
        if not self.kept and hasattr(self, "Xt"):
            del self.Xt, self.rptr, self.ridx           # plain append_rows drops the set
        return out

    def resume_stats(self):
        return dict(leaves_kept=0, block_columns_kept=0, bytes_relocated=0, block_columns_swept=-1, leaves_from_block_0=0,
                    test_set_dropped=0)


def _build(family, X, y, ctx):
    kw = dict(M=30, kernel=dsm.IsoSE(np.log(0.5), 0.0), logNoise=np.log(0.2), ctx=ctx, seed=2)
    if family == "dsmgp":
        return dsm.buildDSMGP(X, y, 2, 4, **kw)
    if family in ("poe", "gpoe"):
        return dsm.buildPoE(X, y, 4, meanFun=None, generalized=family == "gpoe", **kw)
    if family == "rbcm":
        return dsm.buildBCM(X, y, 4, meanFun=None, **kw)
    g = dsm.GaussianProcess(X[:80], y[:80], kernel=kw["kernel"], logNoise=kw["logNoise"], ctx=ctx)
    dsm.fit(g)
    return g


def _predict(family, m, xt):
    return dsm.prediction(m, xt) if family == "gp" else dsm.predict(m, xt)


@pytest.mark.parametrize("family", FAMILIES)
def test_add_data_keeps_the_route_cache_and_registers_nothing_twice(family):
    X, y, xn, yn, xt = _problem(300, 33)
    m, h = _build(family, X, y, KeepingContext()), _build(family, X, y, AppendOracleContext())
    tm = m.model if family == "gp" else m
    _predict(family, m, xt)
    cache = tm._route_cache
    assert cache is not None and cache["uploaded"] and tm.ctx.calls.count("set_test") == 1
    del tm.ctx.calls[:]
    sec = dsm.add_data(m, xn, yn, keep_test=True)
    assert sec.fallback is False and sec.resume_stats == tm.ctx.resume_stats() and tm.ctx.kept
    assert tm._route_cache is cache and cache["uploaded"]
    if family == "dsmgp":
        dsm.update(m)
    mu, var = _predict(family, m, xt)
    assert tm.ctx.calls == ["append_rows keep_test", "predict_run"]          # the same xtest: straight to predict_run
    grow_by_hand(family, h, xn, yn)
    if family == "dsmgp":
        dsm.update(h)
    mo, vo = _predict(family, h, xt)
    assert np.allclose(mu, mo, rtol=1e-12, atol=1e-13) and np.allclose(var, vo, rtol=1e-12, atol=1e-13)
    # another xtest (same shape, other content) is registered
    other = xt[::-1].copy()
    mu2, _ = _predict(family, m, other)
    assert tm.ctx.calls == ["append_rows keep_test", "predict_run", "set_test", "predict_run"]
    assert np.allclose(mu2, _predict(family, h, other)[0], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("family", FAMILIES)
def test_without_the_keyword_every_call_is_what_it_was(family):
    X, y, xn, yn, xt = _problem(300, 34)
    m = _build(family, X, y, KeepingContext())
    tm = m.model if family == "gp" else m
    _predict(family, m, xt)
    del tm.ctx.calls[:]
    sec = dsm.add_data(m, xn, yn)
    assert sec.resume_stats is None and tm._route_cache is None and not tm.ctx.kept
    _predict(family, m, xt)
    assert tm.ctx.calls == ["append_rows", "set_test", "predict_run"]


def test_a_context_without_the_keyword_and_a_dropped_set():
    X, y, xn, yn, xt = _problem(300, 35)
    # a context whose append_rows has no keep_test: the keyword is ignored, the call is today's
    m = _build("dsmgp", X, y, AppendOracleContext())
    dsm.predict(m, xt)
    sec = dsm.add_data(m, xn, yn, keep_test=True)
    assert sec.resume_stats is None and m._route_cache is None and m.ctx.calls[-1] == "append_rows"

    class Dropping(KeepingContext):
        def resume_stats(self):
            return dict(super().resume_stats(), test_set_dropped=1)

    d = _build("dsmgp", X, y, Dropping())
    dsm.predict(d, xt)
    del d.ctx.calls[:]
    sec = dsm.add_data(d, xn, yn, keep_test=True)
    assert sec.resume_stats["test_set_dropped"] == 1 and d._route_cache is not None and d._route_cache["uploaded"] is False
    dsm.predict(d, xt)
    assert d.ctx.calls == ["append_rows keep_test", "set_test", "predict_run"]
    # the fallback after DSMGP_E_NOMEM stays as it is
    f = _build("dsmgp", X, y, KeepingContext())
    dsm.predict(f, xt)
    f.ctx.nomem_next_append = True
    sec = dsm.add_data(f, xn, yn, keep_test=True)
    assert sec.fallback is True and sec.resume_stats is None and f._route_cache is None
