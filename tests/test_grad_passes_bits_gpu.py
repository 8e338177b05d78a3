"""The four hyper-parameter gradient entry points give the bits tests/golden/grad_passes_parent.npz records
(tests/golden/make_grad_passes_parent.py, from the commit before their host code was built from one contraction plan): the
kernels are the same, the task lists are in the same order and the host sums are added in list order, so no tolerance is
involved.  The cases: tests/grad_passes_cases.py."""
import os

import numpy as np
import pytest

import grad_passes_cases as gpc

pytestmark = pytest.mark.gpu

RECORDED = np.load(os.path.join(os.path.dirname(__file__), "golden", "grad_passes_parent.npz"))


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_the_fixture_holds_the_cases_and_nothing_else():
    for k in RECORDED.files:
        assert sum(k.startswith(name + "/") for name in gpc.CASES) == 1, k
    for name in gpc.CASES:
        assert any(k.startswith(name + "/") for k in RECORDED.files), name


@pytest.mark.parametrize("name", list(gpc.CASES))
def test_every_output_is_the_recorded_bits(name):
    got = gpc.run(name)
    want = {k[len(name) + 1:]: RECORDED[k] for k in RECORDED.files if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(got) if not _same_bits(got[k], want[k])]
    for k in bad:
        print(f"\n{name}/{k}: max |difference| {np.max(np.abs(got[k] - want[k])):.3g}")
    assert not bad, (name, bad)
