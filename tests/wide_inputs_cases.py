"""The cases of tests/golden/gp_predgrad_wide.npz and gp_predcov_wide.npz (tests/golden/make_wide_golden.py) as the host and the
GPU tests of the wide inputs read them, and the wrong-index mutant both fixtures are built to catch.  No device."""
import os

import numpy as np

import dense_kernels as dk
import predgrad_dense as pgd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KIND_NAMES = ["isose", "ardse", "isolinear", "ardlinear", "ardseproduct", "isomatern32", "isomatern52", "ardmatern32", "ardmatern52",
              "isorq", "ardrq"]
WIDE_D = (8, 9, 17, 36)
N, NT = 130, 9
PGRAD_DC = 8            # dimensions per round of the input-gradient kernels
COV_STAGE_D = 35        # dimensions per staging round of the covariance epilogue
COV_KINDS = (1, 3, 4, 8, 10)
COV_N, COV_NT, COV_D = 20, 130, 36

ZG = np.load(os.path.join(GOLDEN, "gp_predgrad_wide.npz"))
GRAD_NAMES = sorted(k[:-5] for k in ZG.files if k.endswith("/meta"))


def grad_name(kind, D):
    return f"{KIND_NAMES[kind]}_{N}_{NT}_{D}"


def grad_case(kind, D):
    c = pgd.case_inputs(ZG, grad_name(kind, D))
    assert c["kind"] == kind and c["X"].shape == (N, D) and c["Xt"].shape == (NT, D)
    return c


def cov_cases():
    """{name: case} of gp_predcov_wide.npz, the fields of test_predcov_gpu.CASES plus `ref`, the full symmetric Sigma without noise."""
    cases = dk.load_cases("gp_predcov_wide.npz")
    for c in cases.values():        # meta = kind, mean, logNoise, cond, the pair of the row listed twice
        m = c.pop("meta")
        c.update(kind=int(m[0]), mean=float(m[1]), logNoise=float(m[2]), cond=float(m[3]), dup=(int(m[4]), int(m[5])))
        nt = c["Xt"].shape[0]
        col, row = np.triu_indices(nt)          # the packed lower triangle, column by column (make_predcov_golden.packed_lower)
        c["ref"] = np.zeros((nt, nt))
        c["ref"][row, col] = c["sigma"]
        c["ref"][col, row] = c["sigma"]
    return cases


def first_round_repeated(kind, loghyp, D, per_round):
    """The hyper-vector a kernel sees that indexes its per-dimension factors inside the round only (nh[d] for nh[d0 + d]): the
    length-scales of the first round repeated over all rounds."""
    assert kind in dk.ARD and D > per_round
    h = np.array(loghyp, dtype=np.float64)
    h[:D] = np.resize(h[:per_round], D)
    return h
