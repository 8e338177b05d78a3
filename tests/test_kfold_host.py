"""CPU tests of the k-fold path: the float64 dense helper (tests/kfold_dense.py) against the definition and against its two
extremes, the plan header on the host, the C ABI's declarations and exports, the bindings, make_folds and the substitution of
kfold_predict."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
import dense_gp
import dense_kernels as dk
import kfold_dense as kd
import loo_dense
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel
from pred_tolerance import mll_tol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"dsmgp_kfold": ("int", ["dsmgp_ctx*", "int32_t*", "int32_t", "double*", "double*", "double*", "int32_t*", "double*"]),
       "dsmgp_kfold_seconds": ("int", ["dsmgp_ctx*", "double*"]), "dsmgp_kfold_stats": ("int", ["dsmgp_ctx*", "int64_t*"])}


def _leaf(n, seed=3):
    X, y, _ = dsm.regression_data(n, 2, n_test=4, seed=seed)
    h = np.array([np.log(0.4), 0.0])
    return X, y, dk.value(0, h, X, X), 0.01, float(np.mean(y))


def test_dense_helper_against_the_definition():
    n, K = 60, 4
    X, y, Km, noise, mean = _leaf(n)
    labels = dsm.make_folds(n, K, seed=2)
    labels[::11] = -1
    a = kd.kfold_dense(Km, noise, y, mean, labels, K)
    b = kd.kfold_brute(Km, noise, y, mean, labels, K)
    held = labels >= 0
    assert np.array_equal(np.isnan(a[0]), ~held) and np.array_equal(np.isnan(b[1]), ~held)
    tm, tv = kd.moment_tols(y, b[0], b[1], np.diag(Km), noise)
    assert np.all(np.abs(a[0] - b[0])[held] <= tm[held]) and np.all(np.abs(a[1] - b[1])[held] <= tv[held])
    F = dense_gp.factor(Km, noise)
    cond, normK = kd.factor_stats(F)
    alpha = np.linalg.solve(dk.noisy(Km, noise), y - mean)
    assert np.all(np.abs(a[2] - b[2]) <= 2.0 * kd.lpd_tol_backward(n, cond, alpha, normK))
    assert np.max(np.abs(a[2] - b[2])) < 1e-10 and np.all(np.abs(a[2]) > 1.0)


def test_singletons_are_leave_one_out_and_one_fold_is_the_marginal_likelihood():
    n = 50
    X, y, Km, noise, mean = _leaf(n, seed=8)
    F = dense_gp.factor(Km, noise)
    mu, var, lpd = kd.kfold_from_factor(F, y, mean, np.arange(n), n)
    lm, lv, ll = loo_dense.loo_from_factor(F, y, mean)
    tm, tv, tl, _ = loo_dense.loo_tol(y, lm, lv, np.diag(Km), noise)
    assert np.all(np.abs(mu - lm) <= tm) and np.all(np.abs(var - lv) <= tv) and np.all(np.abs(lpd - ll) <= tl + 1e-13)
    mu, var, lpd = kd.kfold_from_factor(F, y, mean, np.zeros(n, dtype=np.int32), 1)
    gp = dense_gp.DenseGP(0, np.array([np.log(0.4), 0.0, 0.5 * math.log(noise)]), X, y, mean)
    assert abs(lpd[0] - gp.mll()) <= mll_tol(gp.mll(), gp.cond) + 1e-12
    assert np.max(np.abs(mu - mean)) <= 1e-10 and np.max(np.abs(var - np.diag(dk.noisy(Km, noise)))) <= 1e-10
    # an empty label, and rows that are never held out
    mu, var, lpd = kd.kfold_from_factor(F, y, mean, np.where(np.arange(n) % 2, 2, -1), 3)
    assert lpd[0] == 0.0 and lpd[1] == 0.0 and lpd[2] != 0.0 and np.all(np.isnan(mu[::2])) and np.all(np.isfinite(mu[1::2]))


def test_plan_header_on_the_host(tmp_path):
    """csrc/kfold_plan.hpp is plain C++17: tests/kfold_plan_check.cpp, compiled with g++, checks block sizes 1 / 127 / 128 / 129,
    an empty label, label -1, a block whose first row lies in the third row tile, ascending positions inside every block."""
    exe = str(tmp_path / "kfold_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc"),
                    os.path.join(ROOT, "tests", "kfold_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "FAILED" not in run.stdout and run.stdout.rstrip().endswith("all cases passed"), run.stdout + run.stderr
    src = open(os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc", "kfold_plan.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", src).lower()


def _header_prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"\b((?:const\s+)?(?:int64_t|int|char|void|double)\s*\**)\s*(dsmgp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        def norm(t):
            mm = re.match(r"\s*([A-Za-z_]\w*)\s*((?:\*\s*)*)", re.sub(r"\bconst\b", " ", t))
            return mm.group(1) + "*" * mm.group(2).count("*")
        args = m.group(3)
        protos[m.group(2)] = (norm(m.group(1)), [norm(a) for a in args.split(",")] if args.strip() not in ("", "void") else [])
    return protos


def test_header_library_and_bindings_have_the_new_functions():
    protos = _header_prototypes()
    for name, sig in NEW.items():
        assert protos.get(name) == sig, (name, protos.get(name))
        assert name in hipabi.SIGNATURES and len(hipabi.SIGNATURES[name][1]) == len(sig[1])
    if not os.path.exists(hipabi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    out = subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
    assert {s for s in exported if "kfold" in s.lower() and not s.startswith("_Z")} == set(NEW)     # (_Z...: the kernels' host stubs)
    header = open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read()
    for phrase in ("never held out", "NOT counted by dsmgp_estimate_bytes / dsmgp_memory", "depend on its row set only"):
        assert phrase in header, phrase
    julia = open(os.path.join(ROOT, "julia", "DSMGPHip.jl"), encoding="utf-8").read()
    assert ("ccall(sym(:dsmgp_kfold), Cint,\n        (Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, "
            "Ptr{Int32}, Ref{Float64})") in julia
    assert "ccall(sym(:dsmgp_kfold_seconds), Cint, (Ptr{Cvoid}, Ptr{Float64})" in julia
    assert "function kfold(s::Session, fold::AbstractVector{<:Integer}, K::Integer; want_var::Bool=true)" in julia
    export = re.search(r"(?m)^export ([^\n]*)", julia).group(1)
    assert {"kfold", "kfold_seconds"} <= {t.strip() for t in export.split(",")}
    for fn in ("kfold", "kfold_predict", "kfold_scores", "make_folds"):
        assert callable(getattr(dsm, fn))
    assert all(hasattr(c, "kfold") for c in (hipabi.Context, hipabi.MultiContext, hipabi.StreamingContext))


def test_make_folds_is_balanced_deterministic_and_keeps_groups_together():
    f = dsm.make_folds(103, 5, seed=7)
    assert f.dtype == np.int32 and f.shape == (103,) and sorted(np.bincount(f, minlength=5)) == [20, 20, 21, 21, 21]
    assert np.array_equal(f, dsm.make_folds(103, 5, seed=7)) and not np.array_equal(f, dsm.make_folds(103, 5, seed=8))
    assert not np.array_equal(f, np.arange(103) % 5)                # shuffled
    # the portable counter stream: the first labels of this seed are the same on every machine
    order = np.argsort(dsm.datagen.uniform(7, 0, 103), kind="stable")
    assert all(f[order[j]] == j % 5 for j in range(103))
    groups = np.repeat(np.arange(30), 4)[:103]
    g = dsm.make_folds(103, 5, seed=1, groups=groups)
    for v in np.unique(groups):
        assert np.unique(g[groups == v]).size == 1
    assert sorted(np.bincount([g[groups == v][0] for v in np.unique(groups)], minlength=5)) == [5, 5, 5, 5, 6]
    assert np.array_equal(g, dsm.make_folds(103, 5, seed=1, groups=[f"g{v}" for v in groups]))   # group names do not matter
    assert np.array_equal(dsm.make_folds(6, 1), np.zeros(6, dtype=np.int32))
    with pytest.raises(ValueError):
        dsm.make_folds(5, 0)


def test_substitution_of_held_out_moments_on_hand_made_tables():
    """What kfold_predict hands to the aggregation: entries of (leaf, row) pairs whose row the leaf holds AND that has a label
    >= 0 take the held-out moments; rows with label -1 and leaves that never saw the row keep theirs."""
    fold = np.array([0, 1, -1, 0, 1, -1], dtype=np.int32)
    obs = [np.array([4, 0, 2]), np.array([5, 3])]               # leaf 0 holds rows 4, 0, 2 (in that order); leaf 1 rows 5, 3
    mu_k = [np.array([40.0, 0.5, np.nan]), np.array([np.nan, 30.0])]
    var_k = [np.array([4.0, 0.05, np.nan]), np.array([np.nan, 3.0])]
    ptr = np.array([0, 4, 7])                                   # routed entries: leaf 0 sees rows 0, 1, 2, 4; leaf 1 rows 3, 4, 5
    idx = np.array([0, 1, 2, 4, 3, 4, 5])
    mu = np.arange(7, dtype=np.float64) + 100.0
    var = np.arange(7, dtype=np.float64) + 200.0
    o, m, v = dmodel._kfold_held(obs, mu_k, var_k, fold)
    assert [list(a) for a in o] == [[4, 0], [3]] and list(m[0]) == [40.0, 0.5] and list(v[1]) == [3.0]
    smu, svar = dmodel._loo_substitute(ptr, idx, mu, var, o, m, v)
    assert list(smu) == [0.5, 101.0, 102.0, 40.0, 30.0, 105.0, 106.0]
    assert list(svar) == [0.05, 201.0, 202.0, 4.0, 3.0, 205.0, 206.0]
    assert list(mu) == list(np.arange(7) + 100.0)               # copies
