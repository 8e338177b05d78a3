"""CPU tests of the wide-input fixtures (tests/golden/gp_predgrad_wide.npz, gp_predcov_wide.npz): what they cover, the dense
float64 helpers against their 50 digits, and that they can fail a wrong kernel -- the dense helper fed with the length-scales of the
first round of dimensions repeated over all rounds (what a kernel computes that indexes its per-dimension factors with nh[d] in
place of nh[d0 + d]) misses the references by at least 100 tolerances.  That factor is a condition on the INPUTS of the fixtures
(distinct length-scales, far enough apart); it is no tolerance of the device.  No device."""
import os

import numpy as np
import pytest

import dense_kernels as dk
import predgrad_dense as pgd
from dense_gp import DenseGP
from test_predcov_gpu import entry_tol, lib_noise
import wide_inputs_cases as wc

COV = wc.cov_cases()
MUTANT_MARGIN = 100.0


def test_gradient_fixture_covers_every_kind_and_width():
    assert wc.GRAD_NAMES == sorted(wc.grad_name(kind, D) for kind in range(11) for D in wc.WIDE_D)
    for kind in range(11):
        for D in wc.WIDE_D:
            c = wc.grad_case(kind, D)
            nl = D if kind in dk.ARD else 1
            assert c["loghyp"].size == dk.n_hyper(kind, D, noise=False)
            assert np.unique(c["loghyp"][:nl]).size == nl                              # pairwise distinct length-scales
            if kind in dk.RQ:
                assert c["loghyp"][nl] == np.log(1.5)
            assert c["logNoise"] == float(np.log(0.1)) and c["cond"] <= 1e6
            assert abs(c["mean"] - float(np.mean(c["y"]))) > 0.1
            assert np.array_equal(c["Xt"][0], c["X"][wc.N - 1])                        # Delta = 0
            assert c["dup"] == (1, 4) and np.array_equal(c["Xt"][1], c["Xt"][4])
            assert np.array_equal(c["dmu"][1], c["dmu"][4]) and np.array_equal(c["dvar"][1], c["dvar"][4])
            if kind in dk.LINEAR or kind in dk.RQ:
                assert c["far"] == [] and np.all(np.abs(c["Xt"]) < 2.0)
            else:                                                                      # k* underflows: exactly 0
                assert c["far"] == [2, 3] and np.all(c["Xt"][2] == 1e3) and np.all(c["Xt"][3] == -1e3)
                assert np.all(c["dmu"][2:4] == 0.0) and np.all(c["dvar"][2:4] == 0.0)
            live = [r for r in range(wc.NT) if r not in c["far"]]
            assert np.all(c["dmu"][live] != 0.0) and np.all(c["dvar"][live] != 0.0)
    for name in ("gp_predgrad_wide.npz", "gp_predcov_wide.npz"):
        assert os.path.getsize(os.path.join(wc.GOLDEN, name)) <= os.path.getsize(os.path.join(wc.GOLDEN, "gp_pred.npz"))


def _grad_ratios(c, loghyp):
    """Worst |helper - 50 digits| / tolerance of (dmu, dvar), the helper run with `loghyp`, the tolerance that of the case."""
    _, _, hm, hv = pgd.moments(c["kind"], loghyp, c["logNoise"], c["X"], c["y"], c["mean"], c["Xt"])
    tm, tv = pgd.tolerances(c["kind"], c["loghyp"], c["logNoise"], c["X"], c["y"], c["Xt"], c["dmu"], c["dvar"])
    return float(np.max(np.abs(hm - c["dmu"]) / tm)), float(np.max(np.abs(hv - c["dvar"]) / tv)), hm, hv


@pytest.mark.parametrize("kind", range(11))
def test_dense_helper_against_50_digits(kind):
    for D in wc.WIDE_D:
        c = wc.grad_case(kind, D)
        rm, rv, hm, hv = _grad_ratios(c, c["loghyp"])
        print(f"\n{wc.grad_name(kind, D)}: dense err/tol dmu {rm:.3g} dvar {rv:.3g}")
        assert rm <= 1.0 and rv <= 1.0, (D, rm, rv)
        for p in c["far"]:
            assert np.all(hm[p] == 0.0) and np.all(hv[p] == 0.0)


@pytest.mark.parametrize("kind", dk.ARD)
def test_gradient_fixture_fails_a_kernel_that_indexes_inside_the_round(kind):
    for D in (9, 17, 36):
        c = wc.grad_case(kind, D)
        rm, rv, _, _ = _grad_ratios(c, wc.first_round_repeated(kind, c["loghyp"], D, wc.PGRAD_DC))
        print(f"\n{wc.grad_name(kind, D)}: mutant miss / tol dmu {rm:.3g} dvar {rv:.3g}")
        assert rm >= MUTANT_MARGIN and rv >= MUTANT_MARGIN, (D, rm, rv)


def test_covariance_fixture_covers_the_arms_that_read_the_factors():
    assert sorted(COV) == sorted(f"{wc.KIND_NAMES[k]}_d{wc.COV_D}" for k in wc.COV_KINDS)
    for k in wc.COV_KINDS:
        c = COV[f"{wc.KIND_NAMES[k]}_d{wc.COV_D}"]
        assert c["kind"] == k and c["X"].shape == (wc.COV_N, wc.COV_D) and c["Xt"].shape == (wc.COV_NT, wc.COV_D)
        assert wc.COV_D > wc.COV_STAGE_D and wc.COV_NT > 128                           # two staging rounds; tiles (0,0), (1,0), (1,1)
        assert np.unique(c["loghyp"][:wc.COV_D]).size == wc.COV_D
        a, b = c["dup"]
        assert a < 128 <= b and np.array_equal(c["Xt"][a], c["Xt"][b]) and np.array_equal(c["ref"][a], c["ref"][b])
        assert np.array_equal(c["ref"], c["ref"].T) and np.array_equal(np.diag(c["ref"]) <= c["kss"], np.ones(wc.COV_NT, dtype=bool))


def _cov_ratio(c, loghyp):
    g = DenseGP(c["kind"], np.append(loghyp, c["logNoise"]), c["X"], c["y"], c["mean"])
    assert g.info == 0
    return np.abs(g.prediction_cov(c["Xt"], with_noise=False) - c["ref"]) / entry_tol(c["ref"], c["kss"], lib_noise(c["logNoise"]))


@pytest.mark.parametrize("name", sorted(COV))
def test_dense_covariance_against_50_digits(name):
    c = COV[name]
    worst = float(np.max(_cov_ratio(c, c["loghyp"])))
    print(f"\n{name}: dense err/tol {worst:.3g}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(COV))
def test_covariance_fixture_fails_a_kernel_that_indexes_inside_the_round(name):
    """The second staging round holds dimension 35 alone: with its length-scale replaced by that of dimension 0 some entry of the
    off-diagonal tile (rows 128.., columns ..127) misses by at least 100 tolerances."""
    c = COV[name]
    ratio = _cov_ratio(c, wc.first_round_repeated(c["kind"], c["loghyp"], wc.COV_D, wc.COV_STAGE_D))
    worst = float(np.max(ratio[128:, :128]))
    print(f"\n{name}: mutant miss / tol on tile (1,0) {worst:.3g}")
    assert worst >= MUTANT_MARGIN
