"""CPU tests of the device aggregation of the input gradients: the C ABI's declaration and export, the binding's width rule, the
rows of the context's dependency table, and what the model function refuses."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dsmgp_aggregate_gradients_partial", "dsmgp_aggregate_gradients_finish", "dsmgp_aggregate_gradients",
       "dsmgp_aggregate_columns", "dsmgp_aggregate_columns_gradients")


def test_width_of_the_gradient_sums():
    """D planes per moment sum: 3 D mixture, 2 D PoE and gPoE, 2 G D rBCM."""
    for D in (1, 3, 40):
        assert hipabi.agg_gradients_width(hipabi.AGG_MIXTURE, 0, D) == 3 * D
        assert hipabi.agg_gradients_width(hipabi.AGG_POE, 0, D) == 2 * D == hipabi.agg_gradients_width(hipabi.AGG_GPOE, 5, D)
        assert hipabi.agg_gradients_width(hipabi.AGG_RBCM, 3, D) == 6 * D
        for fam, G in ((0, 0), (1, 0), (2, 0), (3, 4)):
            assert hipabi.agg_gradients_width(fam, G, D) == hipabi.agg_width(fam, G) * D


def test_the_header_declares_and_the_library_exports_exactly_the_new_symbols():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dsmgp_hip.h")).read(), flags=re.S)
    protos = re.findall(r"^int (dsmgp_aggregate_(?:gradients|columns)\w*)\(([^;]*)\);", header, flags=re.M)
    assert sorted(n for n, _ in protos) == sorted(NEW)
    for name, args in protos:
        assert name in hipabi.SIGNATURES and len(hipabi.SIGNATURES[name][1]) == args.count(",") + 1
        assert not any(w in name for w in ("target", "append", "loo_columns"))
    dp, i32, i64, ctx = hipabi._dp, hipabi.C.c_int32, hipabi.C.c_int64, hipabi._ctx
    assert hipabi.SIGNATURES[NEW[0]] == (hipabi.C.c_int, [ctx, dp, dp])
    assert hipabi.SIGNATURES[NEW[1]] == (hipabi.C.c_int, [ctx, dp, i32, i32, dp, dp, i64])
    assert hipabi.SIGNATURES[NEW[2]] == (hipabi.C.c_int, [ctx, i32, i32, dp, dp, i64, dp])
    assert hipabi.SIGNATURES[NEW[3]] == (hipabi.C.c_int, [ctx, i32, dp, hipabi._ip, i32, i32, i32, dp, dp, i64, dp])
    assert hipabi.SIGNATURES[NEW[4]] == (hipabi.C.c_int, [ctx, i32, i32, dp, dp, i64, dp])
    out =subprocess.run(["nm", "-D", "--defined-only", hipabi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {n for n in exported if "aggregate_gradients" in n or "aggregate_columns" in n} == set(NEW)


def test_the_dependency_table_has_the_two_rows(tmp_path):
    """csrc/ctx_state.hpp: the per-entry gradients fall with the prediction; the gradient sums fall with them and with the
    aggregated moments (so with new partial sums, a new total, a new prediction, a new fit)."""
    exe = str(tmp_path / "ctx_state_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "deepstructuredmixtures_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ctx_state_dump.cpp"), "-o", exe], check=True)
    table = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True).stdout)
    assert set(table["pred_gradients"]["parents"]) == {"prediction"}
    assert set(table["gradient_sums"]["parents"]) == {"pred_gradients", "done"}
    for p in ("fit", "test", "prediction", "partial", "done", "pred_gradients"):
        assert "gradient_sums" in table[p]["falls"], p
    assert "pred_gradients" in table["prediction"]["falls"] and "pred_gradients" not in table["partial"]["falls"]
    assert not table["gradient_sums"]["falls"] and table["pred_gradients"]["falls"] == ["gradient_sums"]
    for p in ("column_means", "column_mean_gradients"):
        assert set(table[p]["parents"]) == {"prediction", "targets"}
    assert set(table["column_moments"]["parents"]) == {"column_means"} and table["column_means"]["falls"] == ["column_moments"]
    assert "column_moments" in table["targets"]["falls"] and "column_moments" in table["prediction"]["falls"]
    assert "column_moments" not in table["done"]["falls"] and "gradient_sums" not in table["column_means"]["falls"]


def test_keyword_refusals():
    """aggregate= takes "host" or "device"; "device" refuses what the host form refuses, and a context without the call."""
    from oracle_context import OracleContext
    X, y, Xt = dsm.regression_data(300, 2, n_test=5, seed=11)
    kw = dict(M=60, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.1), seed=3)
    model = dsm.buildDSMGP(X, y, 2, 2, ctx=OracleContext(), **kw)
    for bad in ("gpu", None, True, "Device"):
        with pytest.raises(ValueError, match="aggregate must be"):
            dsm.predict_gradients(model, Xt, aggregate=bad)
    gp = dsm.GaussianProcess(X, y, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.1), ctx=OracleContext())
    with pytest.raises(ValueError, match="aggregate must be"):
        dsm.predict_gradients(gp, Xt, aggregate="gpu")
    with pytest.raises(NotImplementedError, match="has no predict_gradients"):
        dsm.predict_gradients(model, Xt, aggregate="device")
    world = model.shard.world
    model.shard.world = 2
    try:
        with pytest.raises(NotImplementedError, match="several ranks"):
            dsm.predict_gradients(model, Xt, aggregate="device")
    finally:
        model.shard.world = world
    node = model.root
    while node.kind != "sum":
        node = node.children[0]
    node.logweights = node.logweights + 0.3
    with pytest.raises(ValueError, match="not normalised"):
        dsm.predict_gradients(model, Xt, aggregate="device")
    stream = dsm.buildDSMGP(X, y, 2, 2, fit_now=False, stream_budget="auto", **kw)
    with pytest.raises(hipabi.DsmgpError) as e:
        dsm.predict_gradients(stream, Xt, aggregate="device")
    assert e.value.code == hipabi.E_STATE
    assert not hasattr(hipabi.StreamingContext, "aggregate_gradients") and hasattr(hipabi.MultiContext, "aggregate_gradients")
    # the column functions: the keyword; contexts without the column calls are refused as by the host form
    multi = dsm.buildDSMGP(X, y, 2, 2, fit_now=False, n_sub=2, **kw)
    for fn in (dsm.predict_targets, dsm.predict_targets_gradients):
        with pytest.raises(ValueError, match="aggregate must be"):
            fn(model, Xt, aggregate="gpu")
        for m in (multi, stream):
            with pytest.raises(NotImplementedError, match="has no solve_targets"):
                fn(m, Xt, aggregate="device")
    assert hasattr(hipabi.Context, "aggregate_columns") and not hasattr(hipabi.MultiContext, "aggregate_columns")
