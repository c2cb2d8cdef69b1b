"""Correspondence rejection (include/s4p_icp_reject.h) on the host: exports and binding, the numpy restatement
(tests/icp_reject_helpers.py) against numpy_brute in both directions, what the filters keep on a partially overlapping pair
and on random normals, the reverse map, the command line's new flags, and the Python argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_reject_helpers as JH
from tests import icp_robust_helpers as RH

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


@pytest.fixture(scope="module")
def bumpy20k():
    from super4pcs_amd import datasets as D
    P, Q, T_gt = D.bumpy_pair(20_000, overlap=0.5, delta=0.004, seed=11)
    c = P.astype(np.float64).mean(0).astype(np.float32)
    return (P - c).astype(np.float32), (Q - c).astype(np.float32), T_gt, c


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def test_reject_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_reject.h")
    assert len(decl) == 4, decl
    assert set(decl) == set(icp_lib.REJECT_SYMBOLS)
    others = (set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS) | set(icp_lib.ROBUST_SYMBOLS) | set(icp_lib.GICP_SYMBOLS)
              | set(icp_lib.COLOR_SYMBOLS))
    assert not set(decl) & others
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    out = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_reject", "k_reject_out"):
        assert re.search(r"s4p_icp::%s\b" % k, out), k
    r = icp_lib.Reject()
    r.reciprocal, r.normal_mode, r.normal_cos = 1, 2, 0.5
    Lb.s4p_icp_reject_defaults(ctypes.byref(r))
    assert (r.reciprocal, r.normal_mode, r.normal_cos) == (0, 0, 0.0) and ctypes.sizeof(r) == 48


def test_reverse_map_is_the_transpose_and_inverts_a_rigid_motion():
    T = RH.motion(7.0, [0.3, -0.2, 0.1]).astype(np.float32)
    Ti = JH.reverse_map(T)
    assert np.array_equal(Ti[:3, :3], T[:3, :3].T) and np.array_equal(Ti[3], [0, 0, 0, 1])
    assert np.max(np.abs(Ti.astype(np.float64) @ T.astype(np.float64) - np.eye(4))) <= 4 * 2.0 ** -24
    assert np.array_equal(JH.reverse_map(np.eye(4)), np.eye(4, dtype=np.float32))
    X = np.random.default_rng(1).normal(size=(50, 3)).astype(np.float32)
    assert np.array_equal(RH.apply_f32(JH.I4, X), X)                    # the identity applies exactly


def _small_pair(seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-0.5, 0.5, size=(1500, 2))
    S = np.column_stack([xy, 0.05 * np.sin(6 * xy[:, 0]) * np.cos(5 * xy[:, 1])])
    Pc = S[xy[:, 0] < 0.15].astype(np.float32)
    Qb = S[xy[:, 0] > -0.15]
    Qc = np.concatenate([Qb, Qb[100:160]]).astype(np.float32)          # partial overlap, shared points, 60 duplicates at the end
    Qc[200:600] += rng.normal(scale=0.004, size=(400, 3)).astype(np.float32)
    return Pc, Qc, rng


@pytest.mark.parametrize("seed", [2, 5])
def test_restatement_agrees_with_numpy_brute_in_both_directions(cpu, seed):
    Pc, Qc, rng = _small_pair(seed)
    d = 0.03
    Np = PH.normalise(rng.normal(size=Pc.shape)); Np[::7] = 0
    Nq = PH.normalise(rng.normal(size=Qc.shape)); Nq[::5] = 0
    for T in (np.eye(4), RH.motion(0.7, [0.004, -0.002, 0.001]), RH.motion(-2.0, [0.0, 0.01, 0.0])):
        T = T.astype(np.float32)
        # forward and backward searches
        fi, fd = H.numpy_brute(Pc, Qc, T, d)
        ci, cd = JH.cpu_search(cpu)(Pc, Qc, T, d)
        assert np.array_equal(fi, ci) and np.array_equal(fd, cd)
        every = np.arange(len(Pc))
        rb = JH.reverse_search(H.numpy_brute, Pc, Qc, T, d, every)
        rc = JH.reverse_search(JH.cpu_search(cpu), Pc, Qc, T, d, every)
        assert np.array_equal(rb, rc) and (rb >= 0).sum() > 100 and (rb < 0).sum() > 100
        for kw in (dict(reciprocal=True), dict(normal_mode=1, normal_cos=0.5), dict(normal_mode=2, normal_cos=0.5),
                   dict(reciprocal=True, normal_mode=1, normal_cos=0.7)):
            a = JH.restate(H.numpy_brute, Pc, Qc, T, d, Np=Np, Nq=Nq, **kw)
            b = JH.restate(JH.cpu_search(cpu), Pc, Qc, T, d, Np=Np, Nq=Nq, **kw)
            for u, v in zip(a, b):
                assert np.array_equal(u, v), kw
            idx, d2, why, counts = a
            assert counts[0] == counts[1] + counts[2] + counts[3] == (fi >= 0).sum()
            assert counts[3] > 50 and counts[1] + counts[2] > 50, (kw, counts)
            assert np.array_equal(idx >= 0, why == JH.KEPT) and np.array_equal(idx[idx >= 0], fi[idx >= 0])
            assert not d2[idx < 0].any() and np.array_equal(d2[idx >= 0], fd[idx >= 0])
            if kw.get("reciprocal"):
                # reciprocity by its definition, through the full reverse map
                kept = np.flatnonzero(why == JH.KEPT)
                assert np.array_equal(rb[fi[kept]], kept)
                lost = np.flatnonzero(why == JH.RECIPROCITY)
                assert np.all(rb[fi[lost]] != lost)
                # of the 60 duplicated source points only the lower index can be kept
                dup_hi = np.arange(len(Qc) - 60, len(Qc))
                assert not np.any(why[dup_hi] == JH.KEPT)


def test_reciprocity_keeps_and_rejects_on_a_half_overlapping_pair(cpu, bumpy20k):
    """bumpy_pair(20 000, overlap 0.5) at d = 4 delta: more than 1000 pairs kept and more than 1000 rejected, at the
    generator's pose and 1 degree / 0.004 off it (two independent samplings of one surface: roughly one pair in three is
    mutual)."""
    Pc, Qc, T_gt, c = bumpy20k
    d = 4 * 0.004
    for ang, sh in ((0.0, 0.0), (1.0, 0.004)):
        T = H.to_centred(RH.motion(ang, sh) @ T_gt, c).astype(np.float32)
        idx, d2, why, counts = JH.restate(JH.cpu_search(cpu), Pc, Qc, T, d, reciprocal=True)
        print("bumpy 20k, %.1f deg off: matched %d, kept %d (%.0f %%)" % (ang, counts[0], counts[3], 100.0 * counts[3] / counts[0]))
        assert counts[3] > 1000 and counts[2] > 1000 and counts[1] == 0
        assert 0.2 < counts[3] / counts[0] < 0.6
        # a kept target is kept once: reciprocity makes the kept pairs one-to-one
        assert len(np.unique(idx[idx >= 0])) == counts[3]


def test_normal_test_keeps_the_expected_share_of_random_normals(cpu, bumpy20k):
    """Independent uniform unit normals on both clouds: |n . m| is uniform on [0, 1], so the unoriented test at 60 degrees
    keeps 1 - cos 60 = 0.5 of the pairs and the oriented test 0.25; within four standard deviations of the binomial."""
    Pc, Qc, T_gt, c = bumpy20k
    d = 4 * 0.004
    rng = np.random.default_rng(21)
    Np, Nq = PH.normalise(rng.normal(size=Pc.shape)), PH.normalise(rng.normal(size=Qc.shape))
    T = H.to_centred(T_gt, c).astype(np.float32)
    cos60 = float(np.cos(np.deg2rad(60.0)))
    for mode, share in ((1, 0.5), (2, 0.25)):
        _, _, why, counts = JH.restate(JH.cpu_search(cpu), Pc, Qc, T, d, normal_mode=mode, normal_cos=cos60, Np=Np, Nq=Nq)
        m = int(counts[0])
        got = counts[3] / m
        tol = 4.0 * np.sqrt(share * (1 - share) / m)
        print("mode %d: kept %.4f of %d pairs, expected %.2f +- %.4f" % (mode, got, m, share, tol))
        assert m > 5000 and abs(got - share) <= tol and counts[2] == 0 and counts[1] == m - counts[3]
    # a zero normal on either side carries no information: the pair is kept
    Nz = Nq.copy(); Nz[::3] = 0
    _, _, why, _ = JH.restate(JH.cpu_search(cpu), Pc, Qc, T, d, normal_mode=2, normal_cos=1.0, Np=Np, Nq=Nz)
    assert np.all(why[::3] != JH.NORMALS) and (why == JH.NORMALS).sum() > 1000


def test_cli_rejection_flags_parse_and_bad_values_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for bad in (["--icp", "30", "--icp-normal-angle", "-1"], ["--icp", "30", "--icp-normal-angle", "91"],
                ["--icp", "30", "--icp-normal-angle", "nan"], ["--icp", "30", "--icp-normal-angle", "6x"],
                ["--icp", "30", "--icp-normal-angle", ""], ["--icp-reciprocal"], ["--icp-normal-angle", "60"],
                ["--icp", "0", "--icp-reciprocal"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-reciprocal" in r.stderr and "--icp-normal-angle" in r.stderr, \
            (bad, r.returncode, r.stderr)
    for good in (["--icp-reciprocal"], ["--icp-normal-angle", "60"], ["--icp-reciprocal", "--icp-normal-angle", "0"],
                 ["--icp-normal-angle", "90", "--icp-metric", "plane"], ["--icp-reciprocal", "--icp-metric", "gicp"],
                 ["--icp-reciprocal", "--icp-normal-angle", "45", "--icp-loss", "trimmed", "--icp-trim", "0.5"],
                 ["--icp-reciprocal", "--icp-loss", "tukey", "--icp-metric", "plane"],
                 ["--icp-reciprocal", "--icp-normal-angle", "60", "--icp-metric", "color"],
                 ["--icp-reciprocal", "--icp-scales", "0.04,0.01,0"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "30"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)


def test_python_argument_checks_need_no_device(icp_lib):
    P = np.zeros((4, 3), np.float32)
    for kw in (dict(normal_angle=-1), dict(normal_angle=91), dict(normal_angle=181, normals_oriented=True),
               dict(normal_angle=float("nan")), dict(normals_oriented=True)):
        with pytest.raises(ValueError):
            icp_lib.refine(P, P, max_distance=1.0, **kw)
    r = icp_lib.reject_params(True, 60.0)
    assert (r.reciprocal, r.normal_mode) == (1, icp_lib.NORMALS_UNORIENTED) and r.normal_cos == np.cos(np.deg2rad(60.0))
    r = icp_lib.reject_params(False, 120.0, oriented=True)
    assert (r.reciprocal, r.normal_mode) == (0, icp_lib.NORMALS_ORIENTED) and r.normal_cos == np.cos(np.deg2rad(120.0))
    assert icp_lib.reject_params(False, 90.0).normal_cos >= 0.0 and icp_lib.reject_params(False, 180.0, True).normal_cos == -1.0
    r = icp_lib.reject_params()
    assert (r.reciprocal, r.normal_mode, r.normal_cos) == (0, 0, 0.0)
    # multiscale forwards the keywords to icp.refine unchanged
    import inspect
    from super4pcs_amd import multiscale
    sig = inspect.signature(icp_lib.refine)
    assert all(k in sig.parameters for k in ("reciprocal", "normal_angle", "normals_oriented"))
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(multiscale.refine_multiscale).parameters.values())
