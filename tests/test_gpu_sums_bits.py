"""GPU: the fp64 sums of every estimation loop, and the ICP states the loops leave, bit for bit against the words recorded in
tests/golden/sums_bits.json (by tests/golden/make_sums_bits.py, at the commit the file names).  The sums are a fixed-order
reduction (csrc/r3d_sums_dev.h: shuffle tree, four waves through LDS, partial rows folded in order); these words pin that order
and the shared state update, so that an edit which reorders one addition in any of the loops fails here.

Cases (tests/sums_bits_cases.py): the 18 pair sums through the separate gather pass (59 partial rows; 274 rows, where finish
threads 0..17 fold two rows each), ungated and gated; the 18 sums taken inside the NN index's cold and warm query kernels and the
state after 3 iterations; the 29 point-to-plane sums for the four parameter sets of test_gpu_plane_icp.py with the state after 3
iterations (48 rows: the plane path caps its rows at the compute-unit count, so its finish never strides); the 29 tracking
sums at 48 x 64 (3 rows) and 480 x 640 (300 rows, strided finish) with their states; the RANSAC refit's 10 sums through every
float of the refined plane and the inlier mask.

The separate pass caps its rows at 4 x compute units, so the words belong to the device the file was recorded on: the first test
demands that compute-unit count."""
import json
import os

import pytest

import sums_bits_cases as SC
from helpers import r3d as _r3d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "sums_bits.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def ctx():
    c = _r3d().Context(0)
    yield c
    c.close()


def test_device_has_the_recorded_compute_units(golden):
    got = SC.compute_units()
    assert got == golden["compute_units"], ("sums_bits.json was recorded on a device with %d compute units, this one reports %d: the "
                                            "separate sums pass launches min(rows, 4 x compute units) workgroups, so its partial rows "
                                            "-- and the last bits of the sums -- differ" % (golden["compute_units"], got))
    assert set(golden["cases"]) == set(SC.CASES)


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_sums_and_states_are_the_recorded_words(golden, ctx, name):
    assert SC.compute_units() == golden["compute_units"], "recorded on a device with another compute-unit count"
    bits, facts = SC.run(name, ctx)
    want = golden["cases"][name]
    assert set(bits) == set(want)
    for key in sorted(want):
        assert bits[key] == want[key], "%s / %s differs from the words recorded at %s" % (name, key, golden["recorded_at_commit"])
    if "rows" in facts and name.startswith("icp_separate"):
        assert facts["rows"] <= 4 * golden["compute_units"]      # the cap is not what set the row count of these cases
