"""GPU tests of the prediction-side kernels past one chunk of input dimensions, with distinct length-scales per dimension:
pred_inputgrad_kernel / pred_inputgrad_rq_kernel (rounds of 8 dimensions), targets_inputgrad_kernel / targets_inputgrad_rq_kernel
(the arm of D > 8) and predcov_epilogue (staging rounds of 35 dimensions) under tile_predcov_kernel and predsample_sigma_kernel.

References: tests/golden/gp_predgrad_wide.npz and gp_predcov_wide.npz (50 digits, tests/golden/make_wide_golden.py);
tests/test_wide_inputs_host.py shows that a kernel which indexes its per-dimension factors inside the round misses them by at
least 100 tolerances.  The checks and tolerances are those of test_predgrad_gpu.py, test_targets_inputgrad_gpu.py,
test_predcov_gpu.py and test_predsample_gpu.py, called as they stand."""
import numpy as np
import pytest

from deepstructuredmixtures_amd import datagen, hipabi
from predsample_dense import check_factor
import test_predcov_gpu as tpc
import test_predgrad_gpu as tpg
import test_targets_inputgrad_gpu as tti
import wide_inputs_cases as wc

pytestmark = pytest.mark.gpu

COV = wc.cov_cases()
JITTER = 1e-8           # dsmgp_predict_sample's default without noise


@pytest.fixture(scope="module")
def ctx():
    c = hipabi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("kind", range(11))
def test_predict_gradients_against_50_digits(ctx, kind, path):
    """D = 8 (exactly one chunk), 9 (a tail of one), 17 (three rounds), 36, n = 130 (a second slab of two training rows): dmu and
    dvar within the tolerance of the 50 digits; the row listed twice, a repeated call and dmu alone (the other instantiation) the
    same bits; the far rows exactly 0."""
    for D in wc.WIDE_D:
        tpg._check_case(ctx, wc.grad_case(kind, D), path, f"{wc.grad_name(kind, D)} {path}")


@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("kind", range(11))
def test_predict_targets_gradients_against_50_digits(ctx, kind, path):
    """The same cases with Q = 3: column 0 (Y[:, 0] = y) within the tolerance of the 50 digits, columns 1 and 2 within twice it of
    the dense helper on the device's own factor; a column solved alone and the Q = 1 call reproduce their bits, and Q = 1 agrees
    with predict_gradients within twice the tolerance."""
    for D in wc.WIDE_D:
        tti._check_case(ctx, wc.grad_case(kind, D), path, f"{wc.grad_name(kind, D)} {path}")


@pytest.mark.parametrize("path", ["standalone", "joint"])
@pytest.mark.parametrize("name", sorted(COV))
def test_covariance_and_sample_factor_at_two_staging_rounds(ctx, name, path):
    """D = 36, n_t = 130 (tiles (0,0), (1,0), (1,1)), one kind per arm that reads the per-dimension factors: Sigma with and
    without noise within the per-entry tolerance of the 50 digits and symmetric to the bit; the factor predict_sample forms
    reproduces Sigma + jitter I by the backward-error criterion of test_predsample_gpu.py."""
    c = COV[name]
    nt = c["Xt"].shape[0]
    noise = tpc.lib_noise(c["logNoise"])
    ref1 = c["ref"] + noise * np.eye(nt)
    tpc._single(ctx, c, path)
    tag = f"{name} {path}"
    S = {False: ctx.predict_cov(0, nt, with_noise=False), True: ctx.predict_cov(0, nt, with_noise=True)}
    tpc._check(tag + " Sigma", S[False], c["ref"], tpc.entry_tol(c["ref"], c["kss"], noise))
    tpc._check(tag + " Sigma + noise", S[True], ref1, tpc.entry_tol(ref1, c["kss"], noise))
    assert tpc._same_bits(S[False], S[False].T) and tpc._same_bits(S[True], S[True].T)
    eps = datagen.normal(77, 0, nt * 3).reshape((nt, 3), order="F")
    for with_noise in (False, True):
        out, info = ctx.predict_sample(eps, with_noise=with_noise)
        assert info[0] == 0 and np.all(np.isfinite(out))
        A = S[with_noise].copy()
        A[np.arange(nt), np.arange(nt)] += 0.0 if with_noise else JITTER
        check_factor(f"{tag} noise={with_noise}", A, ctx.predict_cov_factor(0, nt))
