"""The aggregation entry points and the scores give the bits tests/golden/agg_parent.npz records
(tests/golden/make_agg_parent.py, from the commit before the family rules were stated once in csrc/kernels_agg.hpp): the kernels
perform the same float64 operations in the same order, so no tolerance is involved.  NaN must stand where NaN is recorded (the
payload is not compared).  The cases: tests/agg_bits_cases.py."""
import os

import numpy as np
import pytest

import agg_bits_cases as abc

pytestmark = pytest.mark.gpu

PATH = os.path.join(os.path.dirname(__file__), "golden", "agg_parent.npz")
RECORDED = np.load(PATH)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint64)[ok], b.view(np.uint64)[ok])


def test_the_fixture_holds_the_cases_and_nothing_else():
    assert os.path.getsize(PATH) < (1 << 20)
    for k in RECORDED.files:
        assert sum(k.startswith(name + "/") for name in abc.CASES) == 1, k
    for name in abc.CASES:
        assert any(k.startswith(name + "/") for k in RECORDED.files), name


@pytest.mark.parametrize("name", list(abc.CASES))
def test_every_output_is_the_recorded_bits(name):
    got = abc.run(name)
    want = {k[len(name) + 1:]: RECORDED[k] for k in RECORDED.files if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(got) if not _same_bits(got[k], want[k])]
    for k in bad:
        with np.errstate(all="ignore"):
            print(f"\n{name}/{k}: max |difference| {np.nanmax(np.abs(got[k] - want[k])):.3g}")
    assert not bad, (name, bad)
