"""The facade headers against tests/golden/facade_parity.json: what tests/icp_facade_app (RefineICP with every metric, own and
estimated normals, losses, rejection; RefineICPBatch), multiway_app (RegisterMultiway, ICPInformation), icp_multiscale_app and
normals_facade_app (normals, orient, outliers, voxel) print on the hippo fixture.  The file was recorded on the MI355X by
tests/golden/make_facade_parity_golden.py with the headers as they stood before the session steps were stated once
(DESIGN.md section "Facade: layout"); this test builds the programs from this tree and runs the recorder's own list.  The
headers' host arithmetic has a fixed order and the libraries sum in a fixed order, so the bar is equal strings, line by
line, and an equal exit status."""
import json
import os

import pytest

from tests.golden import make_facade_parity_golden as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    assert os.path.exists(G.OUT), "tests/golden/facade_parity.json is missing"
    with open(G.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def programs(s4p_lib_built, tmp_path_factory):
    from super4pcs_amd import build as B
    B.build_icp()
    B.build_normals()
    return G.build(tmp_path_factory.mktemp("facade_parity_bin"))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return G.write_inputs(tmp_path_factory.mktemp("facade_parity_in"))


def test_the_fixture_holds_the_recorders_cases(golden):
    assert sorted(golden) == sorted(c[0] for c in G.CASES)
    for name, want in golden.items():
        assert want["returncode"] == 0 and want["lines"], name


@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_program_prints_the_recorded_lines(case, golden, programs, files):
    want = golden[case[0]]
    got = G.run_case(case, programs, files)
    for k, (g, w) in enumerate(zip(got["lines"], want["lines"])):
        if g != w:
            print("line %d\n  got  %s\n  want %s" % (k, g, w))
    assert got["returncode"] == want["returncode"]
    assert len(got["lines"]) == len(want["lines"])
    for g, w in zip(got["lines"], want["lines"]):
        assert g == w
