"""`Super4PCS --icp N --icp-starts K` on the hippo fixture the other command-line tests use: the matcher's K best distinct
poses refined in one batch, the matcher's own result first, so the pose kept never has fewer correspondences than --icp
alone finds."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import apps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))



def _matrix(path):
    lines = open(path).read().splitlines()
    assert lines[:2] == ["VERSION\t=\t1", "MATRIX\t="]
    return np.array([[float(v) for v in ln.split()] for ln in lines[2:6]])


def test_icp_starts_runs_and_keeps_at_least_the_single_refinements_correspondences(tmp_path, s4p_lib_built):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    base = [cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "-o", str(overlap), "-d", str(delta), "-t", "1000", "-n", str(n_s),
            "--icp", "10"]
    one = subprocess.run(base + ["-m", str(tmp_path / "one.txt")], capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stderr
    m = re.search(r"ICP: (\d+) iterations, rmse (\S+), fitness (\S+)", one.stdout + one.stderr)
    assert m, one.stdout + one.stderr
    n_one = int(round(float(m.group(3)) * len(Qu)))               # fitness = n_corr / |Q|, printed to six digits; |Q| is a few thousand
    many = subprocess.run(base + ["--icp-starts", "4", "-m", str(tmp_path / "many.txt")], capture_output=True, text=True, timeout=300)
    assert many.returncode == 0, many.stderr
    log = many.stdout + many.stderr
    s = re.search(r"ICP starts: (\d+) of (\d+) candidates", log)
    b = re.search(r"ICP best pose: start (\d+) of (\d+), correspondences (\d+) \(start 0: (\d+)\)", log)
    assert s and b, log
    print(s.group(0), "|", b.group(0), "| --icp alone:", n_one)
    n_starts, best, n_best, n_zero = int(s.group(1)), int(b.group(1)), int(b.group(3)), int(b.group(4))
    assert 1 <= n_starts <= 4 and int(b.group(2)) == n_starts and 0 <= best < n_starts and int(s.group(2)) > 0
    assert n_zero == n_one                                        # start 0 is the refinement --icp alone runs
    assert n_best >= n_one
    M1, M4 = _matrix(tmp_path / "one.txt"), _matrix(tmp_path / "many.txt")
    assert np.all(np.isfinite(M4)) and abs(np.linalg.det(M4[:3, :3]) - 1.0) < 1e-3
    if best == 0:
        assert np.array_equal(M1, M4)
    # with --icp-scales the batch is the coarsest level
    ms = subprocess.run(base + ["--icp-starts", "4", "--icp-scales", "0.05,0", "-m", str(tmp_path / "ms.txt")], capture_output=True,
                        text=True, timeout=300)
    assert ms.returncode == 0, ms.stderr
    assert "ICP best pose: start" in ms.stdout + ms.stderr and "ICP level 1" in ms.stdout + ms.stderr
    assert np.all(np.isfinite(_matrix(tmp_path / "ms.txt")))


def test_icp_starts_with_a_loss_exits_with_the_usage_error(tmp_path, s4p_lib_built):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    r = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "--icp", "10", "--icp-starts", "4", "--icp-loss", "huber"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-starts" in r.stderr
