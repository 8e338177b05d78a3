"""CPU tests of the leave-one-out references: the float64 dense helper (tests/loo_dense.py) against the 50-digit fixture
(tests/golden/gp_loo.npz) and against the brute-force definition (refit without row i, predict at x_i), and the substitution
step of model.loo_predict on hand-made CSR lists."""
import math
import os

import numpy as np
import pytest

import dense_kernels as dk
import loo_dense
from deepstructuredmixtures_amd import hipabi
from deepstructuredmixtures_amd import model as dmodel
from pred_tolerance import moment_tol

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
CASES = loo_dense.load_cases()


def test_fixture_covers_the_cases_the_feature_names():
    ns = {c["X"].shape[0] for c in CASES.values()}
    Ds = {c["X"].shape[1] for c in CASES.values()}
    kinds = {c["kind"] for c in CASES.values()}
    assert {1, 127, 128, 129, 300} <= ns and {1, 8, 40} <= Ds and {0, 1, 3, 8} <= kinds
    assert all(c["mean"] != 0.0 for c in CASES.values())
    assert any(abs(c["mean"] - float(np.mean(c["y"]))) > 0.1 for c in CASES.values())
    assert max(float(np.max(np.abs(c["y"]))) for c in CASES.values()) > 500.0
    assert all(c["cond"] <= 1e6 for c in CASES.values())
    assert os.path.getsize(os.path.join(GOLDEN, "gp_loo.npz")) <= os.path.getsize(os.path.join(GOLDEN, "gp_pred.npz"))


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_helper_against_50_digits(name):
    c = CASES[name]
    noise = math.exp(2.0 * c["logNoise"])
    K = dk.value(c["kind"], c["loghyp"], c["X"], c["X"])
    assert np.all(np.abs(np.diag(K) - c["kss"]) <= 1e-13 * np.maximum(1.0, c["kss"]))
    mu, var, lpd = loo_dense.loo_dense(K, noise, c["y"], c["mean"])
    tm, tv, tl, ts = loo_dense.loo_tol(c["y"], c["mu"], c["var"], c["kss"], noise)
    r = [np.max(np.abs(mu - c["mu"]) / tm), np.max(np.abs(var - c["var"]) / tv), np.max(np.abs(lpd - c["lpd"]) / tl),
         abs(np.sum(lpd) - c["lpd_sum"]) / ts]
    print(f"\n{name}: cond {c['cond']:.3g}, dense err/tol mu {r[0]:.3g} var {r[1]:.3g} lpd {r[2]:.3g} sum {r[3]:.3g}")
    assert max(r) <= 0.01, (name, r)


@pytest.mark.parametrize("kind,n,D", [(0, 60, 2), (3, 75, 3), (8, 90, 4), (0, 1, 1), (1, 2, 2)])
def test_dense_helper_against_brute_force(kind, n, D):
    """The identities behind dsmgp_loo: mu_loo is the mean at x_i of the fit without row i, var_loo its predictive variance
    with noise plus exactly the 1e-8 jitter."""
    rng = np.random.default_rng(100 * kind + n)
    X = rng.uniform(size=(n, D))
    y = np.sin(3.0 * X[:, 0]) + 0.1 * rng.standard_normal(n) + 0.4
    ard = kind in (1, 3, 8)
    loghyp = np.concatenate([np.log(np.full(D if ard else 1, 0.6)), [0.1]])
    noise = 0.1 ** 2
    K = dk.value(kind, loghyp, X, X)
    mean = 0.25
    mu, var, _ = loo_dense.loo_dense(K, noise, y, mean)
    mu_b, var_b = loo_dense.loo_brute(K, noise, y, mean)
    tm, tv = moment_tol(mu_b, var_b, np.diag(K), noise, max(1.0, float(np.max(np.abs(y)))))
    print(f"\nkind {kind} n {n}: mu err/tol {np.max(np.abs(mu - mu_b) / tm):.3g}, "
          f"(var - 1e-8) err/tol {np.max(np.abs((var - loo_dense.JITTER) - var_b) / tv):.3g}")
    assert np.all(np.abs(mu - mu_b) <= tm)
    assert np.all(np.abs((var - loo_dense.JITTER) - var_b) <= tv)


def test_substitution_on_hand_made_lists():
    """Three leaves over five rows.  Leaf 0 predicts rows [0, 1, 2, 3, 4] and observed [3, 1]; leaf 1 predicts [4, 2] and
    observed [2, 4, 0] (row 0 is not routed to it: nothing to replace); leaf 2 predicts [1] and observed nothing."""
    ptr = np.array([0, 5, 7, 8])
    idx = np.array([0, 1, 2, 3, 4, 4, 2, 1])
    mu = np.arange(8, dtype=np.float64)
    var = 10.0 + np.arange(8, dtype=np.float64)
    obs = [np.array([3, 1]), np.array([2, 4, 0]), np.zeros(0, dtype=np.int64)]
    mu_loo = [np.array([-3.0, -1.0]), np.array([-20.0, -40.0, -99.0]), np.zeros(0)]
    var_loo = [np.array([0.3, 0.1]), np.array([0.02, 0.04, 0.99]), np.zeros(0)]
    m, v = dmodel._loo_substitute(ptr, idx, mu, var, obs, mu_loo, var_loo)
    assert m.tolist() == [0.0, -1.0, 2.0, -3.0, 4.0, -40.0, -20.0, 7.0]
    assert v.tolist() == [10.0, 0.1, 12.0, 0.3, 14.0, 0.04, 0.02, 17.0]
    assert mu.tolist() == list(range(8)) and var[0] == 10.0          # the inputs are left alone
    # nothing observed anywhere: nothing changes
    m, v = dmodel._loo_substitute(ptr, idx, mu, var, [np.zeros(0, dtype=np.int64)] * 3, [np.zeros(0)] * 3, [np.zeros(0)] * 3)
    assert np.array_equal(m, mu) and np.array_equal(v, var)


def test_abi_table_and_refusals():
    assert "dsmgp_loo" in hipabi.SIGNATURES
    with open(os.path.join(os.path.dirname(__file__), "..", "include", "dsmgp_hip.h")) as f:
        header = f.read()
    assert "int dsmgp_loo(dsmgp_ctx* ctx" in header and "#define DSMGP_N_TIMINGS 21" in header
    with pytest.raises(hipabi.DsmgpError) as e:
        hipabi.StreamingContext.loo(None)
    assert e.value.code == hipabi.E_STATE
