"""The information matrix (include/s4p_icp_info.h) on the host: exports and binding, the formula of Lambda against the
displacement it measures, and the Python argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import posegraph_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def icp_lib(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp
    return icp


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def _other_lists(icp_lib):
    return (set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS) | set(icp_lib.ROBUST_SYMBOLS) | set(icp_lib.GICP_SYMBOLS) |
            set(icp_lib.SYMM_SYMBOLS) | set(icp_lib.COLOR_SYMBOLS) | set(icp_lib.REJECT_SYMBOLS) | set(icp_lib.BATCH_SYMBOLS))


@pytest.mark.parametrize("header,attr,count", [("s4p_icp_info.h", "INFO_SYMBOLS", 3), ("s4p_icp_posegraph.h", "POSEGRAPH_SYMBOLS", 3)])
def test_new_functions_are_declared_exported_bound_and_disjoint(icp_lib, header, attr, count):
    decl = _declared(header)
    mine = getattr(icp_lib, attr)
    assert decl == sorted(mine) and len(decl) == count, decl
    assert not set(decl) & _other_lists(icp_lib)
    assert not set(icp_lib.INFO_SYMBOLS) & set(icp_lib.POSEGRAPH_SYMBOLS)
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    out = subprocess.run(["nm", "-D", "--defined-only", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    strong = [ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"]
    assert strong and all(s.startswith(("s4p_icp_", "_ZN7s4p_icp")) for s in strong), strong
    assert set(decl) <= set(strong)


def test_info_kernels_are_in_the_library(icp_lib):
    dem = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_info_sum", "k_final_info"):
        assert re.search(r"s4p_icp::%s\b" % k, dem), k
    txt = open(os.path.join(ROOT, "include", "s4p_icp_info.h")).read()
    assert re.search(r"#define S4P_ICP_INFO_NSUMS 11\b", txt) and icp_lib.INFO_NSUMS == 11


@pytest.mark.parametrize("offset", [0.0, 30.0])
def test_lambda_is_the_squared_displacement_to_second_order(icp_lib, offset):
    """xi^T Lambda xi against sum |exp(xi) p - p|^2 (exp: the rotation of omega, then + v) for twists of size 1e-6: the
    two differ in third order, a relative 1e-6; 1e-5 is asserted.  Lambda is the library's: s4p_icp_information_from_sums
    (the host half of s4p_icp_information) on the 11 sums of float32 points p' about a float32 frame c, p = p' + c; it is
    also held to the restatement sum G^T G over p to 1e-12 of the largest entry."""
    assert icp_lib.INFO_NSUMS == 11
    rng = np.random.default_rng(4)
    worst = worst_restated = 0.0
    for k in range(20):
        c = (rng.normal(size=3) * 3 + offset).astype(np.float32)
        pc = rng.uniform(-1, 1, size=(int(rng.integers(3, 300)), 3)).astype(np.float32)
        d2 = rng.uniform(0, 1e-4, size=len(pc)).astype(np.float32)
        pd = pc.astype(np.float64)
        sums = np.concatenate([[len(pc), d2.astype(np.float64).sum()], pd.sum(0),
                               [(pd[:, a] * pd[:, b]).sum() for a in range(3) for b in range(a, 3)]])
        L, n, rmse = icp_lib.information_from_sums(sums, c)
        p = pd + c.astype(np.float64)
        want_L = H.info_from_points(p)
        worst_restated = max(worst_restated, float(np.max(np.abs(L - want_L)) / np.max(np.abs(want_L))))
        assert n == len(pc) and abs(rmse - np.sqrt(sums[1] / n)) <= 1e-15
        assert np.array_equal(L, L.T)
        xi = rng.normal(size=6)
        xi *= 1e-6 / np.linalg.norm(xi)
        D = H.pose(xi[:3], xi[3:])
        moved = p @ D[:3, :3].T + D[:3, 3]
        want = float(((moved - p) ** 2).sum())
        got = float(xi @ L @ xi)
        worst = max(worst, abs(got - want) / want)
    print("offset %g: worst relative |xi^T Lambda xi - sum |dp|^2| %.3g; library against sum G^T G %.3g of the largest entry"
          % (offset, worst, worst_restated))
    assert worst <= 1e-5
    assert worst_restated <= 1e-12
    zero, n0, r0 = icp_lib.information_from_sums(np.zeros(11), np.ones(3, np.float32))
    assert not zero.any() and n0 == 0 and r0 == 0.0


def test_null_arguments_and_python_checks_need_no_device(icp_lib):
    L = icp_lib.load_library()
    assert L.s4p_icp_information_sums(None, None, None) == -1
    assert L.s4p_icp_information(None, None, None, None, None) == -1
    assert L.s4p_icp_information_from_sums(None, None, None, None, None) == -1
    P = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="max_distance"):
        icp_lib.information(P, P, np.eye(4))
    with pytest.raises(ValueError, match="normal_angle"):
        icp_lib.information(P, P, np.eye(4), max_distance=1.0, normal_angle=120)
    from super4pcs_amd import multiway
    with pytest.raises(ValueError, match="max_distance"):
        multiway.register_multiway([P, P])
    with pytest.raises(ValueError, match="metric"):
        multiway.register_multiway([P, P], max_distance=1.0, metric="color")
    with pytest.raises(ValueError, match="pairs"):
        multiway.register_multiway([P, P, P], max_distance=1.0, pairs=[(0, 2)])
    with pytest.raises(ValueError, match="two clouds"):
        multiway.register_multiway([P], max_distance=1.0)


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_headers_compile_with_and_without_eigen_and_the_graph_runs_without_a_device(icp_lib, tmp_path, eigen):
    """tests/multiway_app (algorithms/multiway.h, which includes icp_information.h and posegraph.h) builds with -Werror
    either way.  --check needs no device: OptimizePoseGraph brings a chain whose last node was moved off back to the poses
    that agree with its edges, and an edge with source == target is std::invalid_argument (exit status 5)."""
    import subprocess as sp
    from tests import apps
    extra = ["-I" + os.path.join(ROOT, "oracle", "eigen_shim")] if eigen else ["-DS4P_NO_EIGEN"]
    exe = apps.build_app(tmp_path, "multiway_app", apps.ICP_FACADE_LIBS, ["-Werror"] + extra)
    rng = np.random.default_rng(2)
    poses = [H.random_pose(rng, 0.3, 0.5) for _ in range(4)]
    off = H.pose([0.05, 0, 0.02], [0.1, 0, 0])
    f = tmp_path / "poses.txt"
    f.write_text("".join(" ".join("%.17g" % v for v in X.reshape(16)) + "\n" for X in poses + [off]))
    r = sp.run([exe, str(f), "0.1", "0.3", "--check"], capture_output=True, text=True, timeout=apps.TIMEOUT)
    lines = r.stdout.splitlines()
    assert r.returncode == 5 and lines[-1].startswith("invalid: OptimizePoseGraph"), (r.returncode, r.stdout, r.stderr)
    words = lines[0].split()
    assert words[:2] == ["graph", "iterations"] and int(words[5]) in (1, 3) and int(words[7]) == 0       # converged or stalled at the floor
    assert float(words[10]) <= 1e-18 * float(words[9])
    got = np.array([[float(v) for v in ln.split()[2:18]] for ln in lines[1:5]]).reshape(4, 4, 4)
    assert got[0].tobytes() == np.ascontiguousarray(poses[0]).tobytes()
    assert H.relative_error(got, np.array(poses)) <= 1e-9


def test_cli_information_flag_needs_icp(s4p_lib_built, tmp_path):
    import subprocess as sp
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for bad in (["--icp-information", "f.txt"], ["--icp", "10", "--icp-information"], ["--icp-information", "f.txt", "--icp", "0"]):
        r = sp.run([cli, "-i", "a.obj", "b.obj"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-information file" in r.stderr, (bad, r.returncode, r.stderr)
    r = sp.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "10", "--icp-information", str(tmp_path / "f.txt"),
                "--icp-reciprocal"], capture_output=True, text=True)
    assert r.returncode == 255 and "Can't read input set1" in r.stderr, r.stderr
    head = open(os.path.join(ROOT, "demos", "Super4PCS", "super4pcs_cli.cc")).read().split("#include")[0]
    assert "--icp-information file" in head
