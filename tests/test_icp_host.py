"""ICP refinement (libsuper4pcs_icp.so, include/s4p_icp.h) on the host: exports and binding, the loud failure without a
device, the host solve against numpy, the CPU restatement against a numpy brute force, the command line's new flags."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def icp_lib(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp
    return icp


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def test_icp_library_exports_every_declared_function_and_the_binding_knows_them(icp_lib):
    decl = _declared("s4p_icp.h")
    assert len(decl) == 14, decl
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    assert set(decl) == set(icp_lib.SYMBOLS)
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None or s == "s4p_icp_default_params"


def test_icp_kernels_live_in_their_own_namespace(icp_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "s4p_icp_refine" in out
    # host stubs of the kernels: s4p_icp::k_* only, never the main library's s4p:: namespace
    assert "_ZN3s4p" not in out


def test_icp_create_without_a_gpu_fails_loudly(icp_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: creation succeeds there")
    with pytest.raises(icp_lib.ICPError) as e:
        icp_lib.ICP(0)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def _random_sums(rng, n, R=None, t=None, spread=(1.0, 1.0, 1.0), noise=1e-3):
    q = rng.normal(size=(n, 3)) * np.asarray(spread)
    if R is None:
        A = rng.normal(size=(3, 3)); U, _, Vt = np.linalg.svd(A); R = U @ Vt
        if np.linalg.det(R) < 0:
            R[:, 0] *= -1
    t = rng.normal(size=3) if t is None else t
    p = q @ R.T + t + rng.normal(scale=noise, size=q.shape)
    s = np.zeros(17)
    s[0] = n; s[1:4] = q.sum(0); s[4:7] = p.sum(0); s[7:16] = (q.T @ p).reshape(9); s[16] = 1.0
    return s


def _numpy_solutions(s):
    n = s[0]; mq = s[1:4] / n; mp = s[4:7] / n
    S = s[7:16].reshape(3, 3) / n - np.outer(mq, mp)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    N = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx], [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                  [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy], [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    _, V = np.linalg.eigh(N)
    w, x, y, z = V[:, -1]
    Rh = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    U, _, Vt = np.linalg.svd(S)                               # Kabsch: R = V diag(1, 1, det) U^T
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    Rk = Vt.T @ D @ U.T
    out = []
    for R in (Rh, Rk):
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = mp - R @ mq
        out.append(T)
    return out


@pytest.mark.parametrize("case", ["random", "few_points", "near_planar", "tiny_rotation", "large_offset"])
def test_icp_solve_equals_numpy_eigh_and_kabsch(icp_lib, case):
    rng = np.random.default_rng(hash(case) & 0xFFFF)
    for _ in range(20):
        if case == "random":
            s = _random_sums(rng, 200)
        elif case == "few_points":
            s = _random_sums(rng, 3, noise=0.0)
        elif case == "near_planar":
            s = _random_sums(rng, 500, spread=(1.0, 1.0, 1e-4))
        elif case == "tiny_rotation":
            a = 1e-7
            R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            s = _random_sums(rng, 300, R=R, t=np.zeros(3), noise=0.0)
        else:
            s = _random_sums(rng, 300, t=np.array([50.0, -20.0, 10.0]))
        got = icp_lib.solve(s)
        Th, Tk = _numpy_solutions(s)
        assert np.max(np.abs(got - Th)) <= 1e-12 * max(1.0, np.max(np.abs(Th))), case
        assert np.max(np.abs(got - Tk)) <= 1e-12 * max(1.0, np.max(np.abs(Tk))), case
        R = got[:3, :3]
        assert np.max(np.abs(R @ R.T - np.eye(3))) <= 1e-13 and abs(np.linalg.det(R) - 1.0) <= 1e-13
    with pytest.raises(icp_lib.ICPError):
        icp_lib.solve(np.zeros(17))


def _tie_cloud(rng, n_p, n_q, d):
    """Centred clouds with duplicated target points (ties) and source points exactly at d and just beyond it."""
    P = rng.uniform(-0.5, 0.5, size=(n_p, 3)).astype(np.float32)
    P[n_p // 2:n_p // 2 + n_p // 10] = P[:n_p // 10]                 # duplicates: ties between i and i + n_p / 2
    Q = (P[rng.integers(0, n_p, n_q)] + rng.normal(scale=d / 3, size=(n_q, 3))).astype(np.float32)
    k = n_q // 8
    dd = np.float32(d)
    Q[:k] = P[:k] + np.array([dd, 0, 0], np.float32)                  # x offset fl(p + d): often exactly d apart
    Q[k:2 * k] = P[k:2 * k] + np.array([0, np.nextafter(dd, np.float32(1)), 0], np.float32)   # just beyond
    return P, Q


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_icp_cpu_restatement_equals_numpy_brute_force(cpu, seed):
    rng = np.random.default_rng(seed)
    d = 0.03125 if seed == 1 else 0.021
    P, Q = _tie_cloud(rng, 1500, 800, d)
    for T in (np.eye(4), _small_motion(rng, 0.01, 0.005)):
        i_np, d_np = H.numpy_brute(P, Q, T, d)
        i_gr, d_gr, sums = cpu.pass_(P, Q, T, d)
        i_bf, d_bf = cpu.brute(P, Q, T, d)
        assert np.array_equal(i_np, i_gr) and np.array_equal(d_np, d_gr)
        assert np.array_equal(i_np, i_bf) and np.array_equal(d_np, d_bf)
        assert sums[0] == np.count_nonzero(i_np >= 0)
        assert np.count_nonzero(i_np >= 0) > 100 and np.count_nonzero(i_np < 0) > 0
    # the constructed cases really exercise the edges: a tie and a distance exactly at d
    i_np, d_np = H.numpy_brute(P, Q, np.eye(4), d)
    assert np.any(i_np[:len(Q) // 8] >= 0) and np.any(d_np == np.float32(d) * np.float32(d))


def _small_motion(rng, angle, shift):
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = rng.normal(size=3) * shift
    return T


def test_cli_icp_flags_parse_and_bad_values_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for bad in (["--icp", "abc"], ["--icp", "-3"], ["--icp", "2x"], ["--icp-dist", "0"], ["--icp-dist", "nan"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp" in r.stderr, (bad, r.returncode, r.stderr)
    # well-formed flags parse: the run goes on to read the inputs (missing here: exit -1 like any run)
    r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "30", "--icp-dist", "0.04"],
                       capture_output=True, text=True)
    assert r.returncode == 255 and "Can't read input set1" in r.stderr
