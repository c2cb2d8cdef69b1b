"""Normal estimation (include/s4p_normals.h, libsuper4pcs_normals.so) on the host: exports and binding, the library's
namespace, the loud failure without a device, the CPU restatement's neighbour sets against a numpy lexsort brute force and
its normals against numpy eigh, the command line's new flags and the facade header."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import normals_helpers as NH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nrm():
    from super4pcs_amd import build as B
    B.build_normals()
    from super4pcs_amd import normals
    return normals


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("normals_cpu"))


def _gpu_visible():
    from tests.conftest import _gpu_visible as g
    return g()


def test_header_declarations_equal_the_binding_and_the_exports(nrm):
    txt = open(os.path.join(ROOT, "include", "s4p_normals.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = sorted(set(re.findall(r"\b(s4p_normals_\w+)\s*\(", txt)))
    assert decl == sorted(nrm.SYMBOLS), decl
    L = ctypes.CDLL(nrm.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = nrm.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None, s


def test_kernels_live_in_their_own_namespace(nrm):
    dyn = subprocess.run(["nm", "-D", "--defined-only", nrm.LIB_PATH], capture_output=True, text=True).stdout
    assert "_ZN3s4p" not in dyn
    out = subprocess.run(["nm", "-C", nrm.LIB_PATH], capture_output=True, text=True).stdout
    assert "s4p_icp::" not in out
    for k in ("k_normals", "k_match", "k_final", "k_match_plane", "k_final_plane", "k_stats"):
        assert not re.search(r"\b%s\b" % k, out), k
    assert re.search(r"s4p_nrm::k_knn_normals<8>", out) and re.search(r"s4p_nrm::k_knn_normals<32>", out)
    # only the HIP runtime (and the C / C++ runtimes) are linked
    needed = subprocess.run(["readelf", "-d", nrm.LIB_PATH], capture_output=True, text=True).stdout
    assert "super4pcs" not in needed


@pytest.mark.skipif(_gpu_visible(), reason="checks the failure without a device")
def test_create_fails_loudly_without_a_device(nrm):
    with pytest.raises(nrm.NormalsError) as e:
        nrm.Normals(0)
    assert e.value.code == -2 and "no HIP device" in str(e.value)
    with pytest.raises(nrm.NormalsError):
        nrm.estimate_normals(np.zeros((10, 3), np.float32))


def _cloud_with_ties(rng, n):
    """A small lattice-like cloud: integer coordinates (many exactly equal distances), duplicated points."""
    P = rng.integers(0, 6, size=(n, 3)).astype(np.float32) * np.float32(0.25)
    P[n // 3:n // 3 + n // 10] = P[:n // 10]
    return P


@pytest.mark.parametrize("k,radius", [(3, None), (8, None), (16, 0.6), (32, None), (32, 0.3)])
def test_restatement_neighbour_sets_equal_numpy_lexsort(cpu, k, radius):
    rng = np.random.default_rng(k)
    P = _cloud_with_ties(rng, 400)
    idx, cnt = cpu.knn(P, k, radius)
    ib, cb = NH.numpy_knn(P, k, radius)
    assert np.array_equal(cnt, cb) and np.array_equal(idx, ib)
    # the first neighbour is at d2 = 0: the point itself or a duplicate of smaller index
    assert np.array_equal(P[idx[:, 0]], P) and np.all(idx[:, 0] <= np.arange(len(P)))
    # separate queries, some off the cloud
    Q = np.concatenate([P[:50] + np.float32(0.125), rng.uniform(-1, 2, size=(30, 3)).astype(np.float32)])
    idx, cnt = cpu.knn(P, k, radius, queries=Q)
    ib, cb = NH.numpy_knn(P, k, radius, queries=Q)
    assert np.array_equal(cnt, cb) and np.array_equal(idx, ib)


def test_restatement_normals_agree_with_numpy_eigh(cpu):
    rng = np.random.default_rng(5)
    n = 3000
    xy = rng.uniform(-1, 1, size=(n, 2))
    z = 0.1 * np.sin(2 * xy[:, 0]) + 0.05 * np.cos(3 * xy[:, 1]) + rng.normal(scale=0.003, size=n)
    P = np.column_stack([xy, z]).astype(np.float32)
    for k, radius in ((8, None), (16, None), (32, 0.2)):
        N = cpu.normals(P, k, radius)
        idx, cnt = cpu.knn(P, k, radius)
        P64 = P.astype(np.float64)
        checked = 0
        for i in range(0, n, 7):
            nb = idx[i, :cnt[i]]
            if len(nb) < 3:
                assert not N[i].any()
                continue
            e = P64[nb] - P64[i]
            m = e.mean(0)
            Cm = e.T @ e / len(e) - np.outer(m, m)
            w, V = np.linalg.eigh(Cm)
            if not w[1] >= 4 * max(w[0], 1e-30):
                continue                                      # well-conditioned neighbourhoods only
            v = V[:, 0]
            v = v * (1 if v[np.argmax(np.abs(v))] > 0 else -1)
            assert np.max(np.abs(N[i].astype(np.float64) - v)) <= 1e-6, (i, N[i], v)
            checked += 1
        assert checked > 200
        assert np.all(np.abs(np.linalg.norm(N[N.any(1)].astype(np.float64), axis=1) - 1) < 1e-6)


def test_restatement_zero_normals(cpu):
    P = np.array([[0, 0, 0], [1, 0, 0], [5, 5, 5], [5, 5, 5], [5, 5, 5]], np.float32)
    N = cpu.normals(P, 3, 1.5)
    assert not N.any()                               # fewer than 3 within r, or all coincident (trace 0)
    N = cpu.normals(P, 3)
    assert not N[2:].any()


def test_cli_estimate_normals_flags(tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    base = [cli, "-i", "a.obj", "b.obj"]
    for bad in (["--estimate-normals", "2"], ["--estimate-normals", "33"], ["--estimate-normals", "16.5"], ["--estimate-normals", "x"],
                ["--estimate-normals", ""], ["--estimate-normals", "16", "--estimate-normals-radius", "0"],
                ["--estimate-normals", "16", "--estimate-normals-radius", "-1"],
                ["--estimate-normals", "16", "--estimate-normals-radius", "nan"],
                ["--estimate-normals", "16", "--estimate-normals-radius", "0.1x"], ["--estimate-normals-radius", "0.1"]):
        r = subprocess.run(base + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--estimate-normals" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (["--estimate-normals", "3"], ["--estimate-normals", "32", "--estimate-normals-radius", "0.05"],
                 ["--estimate-normals-radius", "0.05", "--estimate-normals", "16"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj")] + good, capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)


@pytest.mark.skipif(_gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for name in ("P.obj", "Q.obj"):
        with open(tmp_path / name, "w") as f:
            for p in np.random.default_rng(1).uniform(size=(50, 3)):
                f.write("v %.6f %.6f %.6f\n" % tuple(p))
    r = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "--estimate-normals", "16", "-a", "20",
                        "-m", str(tmp_path / "m.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 254, (r.returncode, r.stdout, r.stderr)
    assert "Unknown flag" not in r.stderr and "EstimateNormals (MI355X)" in r.stdout + r.stderr and "no HIP device" in r.stdout + r.stderr


def test_facade_header_compiles_in_a_small_app(nrm, tmp_path):
    exe = apps.build_app(tmp_path, "normals_app", ("super4pcs_normals",), ("-Werror",))
    assert os.path.exists(exe)
