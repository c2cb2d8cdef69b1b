"""libsuper4pcs_icp.so against tests/golden/icp_parity.npz: the sums of every metric, the refine loop's bookkeeping (the
returned transform, every byte of the Result, the robust info) on the max-iterations, converged, too-few and degenerate
paths, and the rejection's answers and counters, with the rejection off and on.  The file was recorded on the MI355X by
tests/golden/make_icp_parity_golden.py, whose record() this test runs again.  Every sum is a fixed-order double sum with no
floating atomics, so the bar is equal bits: np.array_equal, no tolerance."""
import os

import numpy as np
import pytest

from tests.golden import make_icp_parity_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp as I
    return I


def test_every_recorded_array_is_reproduced(icp):
    assert os.path.exists(G.OUT), "tests/golden/icp_parity.npz is missing"
    want = dict(np.load(G.OUT))
    got = G.record(icp)
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(want) if not (got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]))]
    for k in bad[:8]:
        print(k, "\n  got ", got[k], "\n  want", want[k])
    assert not bad, "%d of %d arrays differ: %s" % (len(bad), len(want), bad[:20])
