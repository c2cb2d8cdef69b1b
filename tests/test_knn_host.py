"""Neighbour lists and outlier removal (include/s4p_knn.h, libsuper4pcs_normals.so) on the host: the header's declarations
against the binding and the exports, s4p_normals.h and its symbol list untouched, the new kernels in the library's
namespace, the loud failure without a device, the restatement's lists against the numpy brute force on the tiny shapes of
the GPU tests, the reference statistics, the command line's new flags and the facade header with and without Eigen."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import knn_helpers as KH
from tests import normals_helpers as NH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def knn():
    from super4pcs_amd import build as B
    B.build_normals()
    from super4pcs_amd import knn
    return knn


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("knn_cpu"))


def _gpu_visible():
    from tests.conftest import _gpu_visible as g
    return g()


def _declared(header, prefix):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(%s\w+)\s*\(" % prefix, txt)))


def test_header_declarations_equal_the_binding_and_the_exports(knn):
    decl = _declared("s4p_knn.h", "s4p_(?:knn|outliers)_")
    assert len(decl) == 8 and decl == sorted(knn.SYMBOLS), decl
    assert not _declared("s4p_knn.h", "s4p_normals_")                       # the new functions carry their own prefixes
    from super4pcs_amd import normals
    L = ctypes.CDLL(normals.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = knn.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None and getattr(Lb, s).restype is ctypes.c_int32, s
    exported = subprocess.run(["nm", "-D", "--defined-only", normals.LIB_PATH], capture_output=True, text=True).stdout
    got = sorted(set(re.findall(r"\b(s4p_(?:knn|outliers)_\w+)", exported)))
    assert got == decl, got
    assert ctypes.sizeof(knn.OutlierStats) == 40


def test_the_normals_header_and_its_symbol_list_are_unchanged(knn):
    from super4pcs_amd import normals
    assert _declared("s4p_normals.h", "s4p_normals_") == sorted(normals.SYMBOLS) and len(normals.SYMBOLS) == 10
    digest = hashlib.sha256(open(os.path.join(ROOT, "include", "s4p_normals.h"), "rb").read()).hexdigest()
    # the header as of the scale limit in its Limits paragraph: a comment grew, no declaration changed
    assert digest == "f5f72bed94da6af3e2c3cfa3c129249e091cc62eff74a555a0d401bb0a9d2f22", digest
    assert not [s for s in knn.SYMBOLS if s.startswith("s4p_normals_")]


def test_new_kernels_live_in_the_library_namespace(knn):
    from super4pcs_amd import normals
    out = subprocess.run(["nm", "-C", normals.LIB_PATH], capture_output=True, text=True).stdout
    for k in (8, 16, 32):
        for mode in (0, 1, 2):
            assert re.search(r"s4p_nrm::k_knn_search<%d, %d>" % (k, mode), out), (k, mode)
        assert re.search(r"s4p_nrm::k_knn_normals<%d>" % k, out), k
    for name in ("k_sor_rows<0>", "k_sor_rows<1>", "k_sor_reduce", "k_sor_mask"):
        assert "s4p_nrm::" + name in out, name


@pytest.mark.skipif(_gpu_visible(), reason="checks the failure without a device")
def test_create_fails_loudly_without_a_device(knn):
    with pytest.raises(knn.NormalsError) as e:
        knn.Knn(0)
    assert e.value.code == -2 and "no HIP device" in str(e.value)
    X = np.zeros((10, 3), np.float32)
    for call in (lambda: knn.knn(X, 4), lambda: knn.remove_statistical_outliers(X), lambda: knn.remove_radius_outliers(X, 0.1, 2)):
        with pytest.raises(knn.NormalsError) as e:
            call()
        assert e.value.code == -2


@pytest.mark.parametrize("n", KH.TINY_N)
@pytest.mark.parametrize("dup", [False, True])
def test_restatement_lists_equal_numpy_on_the_tiny_shapes(cpu, n, dup):
    X = KH.tiny_cloud(n, dup)
    for k in (1, 2, 8, 31, 32):
        for r in (None, KH.tiny_radius(n)):
            for ex in (False, True):
                ic, dc, cc = KH.cpu_lists(cpu, X, k, r, exclude_self=ex)
                inp, dn, cn = KH.numpy_lists(X, k, r, exclude_self=ex)
                assert np.array_equal(ic, inp) and np.array_equal(cc, cn) and np.array_equal(KH.bits(dc), KH.bits(dn)), (n, dup, k, r, ex)
                if r is None:
                    assert (cn == min(k, n - 1 if ex else n)).all()
                if not ex:
                    assert (dn[:, 0] == 0).all() and (inp[:, 0] <= np.arange(n)).all()      # itself, or a duplicate of smaller index
                else:
                    assert not (inp == np.arange(n)[:, None]).any()


def test_lists_without_self_keep_duplicates():
    X = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32)
    idx, d2, cnt = KH.numpy_lists(X, 2, exclude_self=True)
    assert idx.tolist() == [[2, 3], [0, 2], [0, 3], [0, 2]] and d2[0].tolist() == [0, 0] and cnt.tolist() == [2, 2, 2, 2]
    m = KH.mean_dist(d2, cnt)
    assert m.tolist() == [0.0, 1.0, 0.0, 0.0]
    mu, sigma, t = KH.sor_reference(m, 2.0)
    assert mu == 0.25 and sigma == 0.5 and t == 1.25
    assert KH.sor_reference(np.zeros(1), 2.0) == (0.0, 0.0, 0.0)


def test_planted_points_are_outliers_of_the_reference(cpu):
    """The reference statistics on the small bumpy cloud of the GPU test, k = 16: every original point is kept, at least 51
    of the 60 planted points are removed, and no m_j lies within 1e-9 (relative) of the threshold."""
    from super4pcs_amd import datasets as D
    X, planted = KH.plant(D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0], 60)
    assert len(X) == 6060 and planted.sum() == 60
    _, d2, cnt = KH.cpu_lists(cpu, X, 16, exclude_self=True)
    m = KH.mean_dist(d2, cnt)
    mu, sigma, t = KH.sor_reference(m, 2.0)
    keep = m <= t
    gap = np.min(np.abs(m - t)) / t
    print("bumpy + 60, k 16: mu %.6g sigma %.6g t %.6g, gap %.3g, planted removed %d" % (mu, sigma, t, gap, (~keep[planted]).sum()))
    assert gap > 1e-9 and keep[~planted].all() and (~keep[planted]).sum() >= 51


def test_cli_remove_outliers_flags(tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    base = [cli, "-i", "a.obj", "b.obj"]
    for bad in (["--remove-outliers", "0"], ["--remove-outliers", "33"], ["--remove-outliers", "1.5"], ["--remove-outliers", "x"],
                ["--remove-outliers", ""], ["--remove-outliers-std", "2.0"], ["--remove-outliers", "16", "--remove-outliers-std", "-1"],
                ["--remove-outliers", "16", "--remove-outliers-std", "nan"], ["--remove-outliers", "16", "--remove-outliers-std", "2x"]):
        r = subprocess.run(base + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--remove-outliers" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (["--remove-outliers", "1"], ["--remove-outliers", "32", "--remove-outliers-std", "0"],
                 ["--remove-outliers-std", "1.5", "--remove-outliers", "16"],
                 ["--remove-outliers", "16", "--estimate-normals", "16", "--icp", "5", "--icp-metric", "gicp"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj")] + good, capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)


def test_cli_refuses_an_input_with_faces(tmp_path):
    """Faces index the vertex list: refused before any device work, with exit status -2."""
    from super4pcs_amd import build as B
    cli = B.build_cli()
    pts = np.random.default_rng(1).uniform(size=(50, 3))
    KH.write_obj(tmp_path / "P.obj", pts)
    KH.write_obj(tmp_path / "Q.obj", pts, faces=[(1, 2, 3), (2, 3, 4)])
    for first, second in (("P.obj", "Q.obj"), ("Q.obj", "P.obj")):
        r = subprocess.run([cli, "-i", str(tmp_path / first), str(tmp_path / second), "--remove-outliers", "16", "-m", str(tmp_path / "m.txt")],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 254 and "faces" in r.stdout + r.stderr, (r.returncode, r.stdout, r.stderr)
        assert not (tmp_path / "m.txt").exists()


@pytest.mark.skipif(_gpu_visible(), reason="checks the failure without a device")
def test_cli_valid_command_fails_with_the_device_error_without_a_gpu(tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    pts = np.random.default_rng(1).uniform(size=(50, 3))
    KH.write_obj(tmp_path / "P.obj", pts); KH.write_obj(tmp_path / "Q.obj", pts)
    r = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "--remove-outliers", "16", "-m", str(tmp_path / "m.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 254, (r.returncode, r.stdout, r.stderr)
    assert "Unknown flag" not in r.stderr and "RemoveOutliers (MI355X)" in r.stdout + r.stderr and "no HIP device" in r.stdout + r.stderr


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(knn, tmp_path, eigen):
    extra = ["-I" + os.path.join(ROOT, "oracle", "eigen_shim")] if eigen else ["-DS4P_NO_EIGEN"]
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "super4pcs/algorithms/outliers.h"\n#ifdef S4P_HAVE_EIGEN\n#error have\n#else\n#error none\n#endif\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + extra + [str(probe)],
                       capture_output=True, text=True)
    assert re.search(r"#error (have|none)", r.stderr).group(1) == ("have" if eigen else "none"), r.stderr
    exe = KH.build_app(tmp_path, extra)
    assert os.path.exists(exe)
    if not _gpu_visible():
        np.savetxt(tmp_path / "P.xyz", np.random.default_rng(2).uniform(size=(20, 3)), fmt="%.6f")
        r = subprocess.run([exe, str(tmp_path / "P.xyz"), "stat", "8", "2.0"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
    for bad in (["stat", "0", "2.0"], ["stat", "33", "2.0"], ["stat", "8", "-1"], ["radius", "-1", "4"], ["radius", "0.1", "33"]):
        np.savetxt(tmp_path / "P.xyz", np.random.default_rng(2).uniform(size=(20, 3)), fmt="%.6f")
        r = subprocess.run([exe, str(tmp_path / "P.xyz")] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "RemoveOutliers:" in r.stderr, (bad, r.stderr)
