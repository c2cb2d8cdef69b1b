"""Batched multi-start ICP (include/s4p_icp_batch.h) on the host: the exports and the binding, the ranking rule against a
numpy restatement, the argument checks that need no device, TopPoses (include/super4pcs/algorithms/icp_batch.h) through a
stand-alone program, plain and under the address and undefined-behaviour sanitizers, and the command line's new flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import apps

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


def test_batch_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_batch.h")
    assert decl == ["s4p_icp_rank_batch", "s4p_icp_refine_batch", "s4p_icp_sums_batch"]
    assert set(decl) == set(icp_lib.BATCH_SYMBOLS)
    others = (set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS) | set(icp_lib.ROBUST_SYMBOLS) | set(icp_lib.GICP_SYMBOLS)
              | set(icp_lib.COLOR_SYMBOLS) | set(icp_lib.REJECT_SYMBOLS))
    assert not set(decl) & others
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    out = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_match_batch<false>", "k_match_batch<true>", "k_final_batch<false>", "k_final_batch<true>"):
        assert "s4p_icp::" + k in out, k
    assert icp_lib.BATCH_MAX == 64 and ctypes.sizeof(icp_lib.BatchParams) == ctypes.sizeof(icp_lib.Params) + 8
    assert "#define S4P_ICP_BATCH_MAX 64" in open(os.path.join(ROOT, "include", "s4p_icp_batch.h")).read()


def _rank_numpy(n_corr, rmse):
    """n_corr descending, then rmse ascending, then the index; poses without a correspondence last, by index."""
    idx = list(range(len(n_corr)))
    have = sorted([i for i in idx if n_corr[i] > 0], key=lambda i: (-int(n_corr[i]), float(rmse[i]), i))
    return np.array(have + [i for i in idx if n_corr[i] <= 0], np.int32)


def _results(icp, n_corr, rmse):
    out = []
    for n, r in zip(n_corr, rmse):
        res = icp.Result()
        res.n_corr, res.rmse = int(n), float(r)
        out.append(res)
    return out


def test_rank_batch_against_the_numpy_restatement(icp_lib):
    rng = np.random.default_rng(5)
    cases = [
        ([5, 7, 7, 3], [0.1, 0.2, 0.1, 0.0]),                       # a tie in n_corr, decided by rmse
        ([7, 7, 7, 7], [0.2, 0.1, 0.2, 0.1]),                       # ties in n_corr and in rmse: the index decides
        ([0, 0, 0], [0.3, 0.1, 0.2]),                               # nothing matched anywhere: by index, whatever the rmse says
        ([0, 4, 0, 9, 0], [0.0, 0.5, 0.0, 0.9, 0.0]),               # the empty ones last, by index
        ([12], [0.4]),                                              # B = 1
        (list(rng.integers(0, 6, 64) * 100), list(rng.integers(0, 4, 64) / 8.0)),      # B = 64, many ties of both kinds
        (list(rng.integers(1, 10 ** 9, 64)), list(rng.random(64))),
    ]
    for n_corr, rmse in cases:
        got = icp_lib.rank_batch(_results(icp_lib, n_corr, rmse))
        want = _rank_numpy(n_corr, rmse)
        assert np.array_equal(got, want), (n_corr, rmse, got, want)
        assert sorted(got) == list(range(len(n_corr)))
    assert list(icp_lib.rank_batch(_results(icp_lib, [5, 7, 7, 3], [0.1, 0.2, 0.1, 0.0]))) == [2, 1, 0, 3]
    assert list(icp_lib.rank_batch(_results(icp_lib, [0, 0, 0], [0.3, 0.1, 0.2]))) == [0, 1, 2]


def test_rank_batch_refuses_bad_sizes_and_null_pointers(icp_lib):
    L = icp_lib.load_library()
    arr = (icp_lib.Result * 65)()
    order = (ctypes.c_int32 * 65)()
    assert L.s4p_icp_rank_batch(arr, 0, order) == -1
    assert L.s4p_icp_rank_batch(arr, 65, order) == -1
    assert L.s4p_icp_rank_batch(arr, -3, order) == -1
    assert L.s4p_icp_rank_batch(None, 4, order) == -1
    assert L.s4p_icp_rank_batch(arr, 4, None) == -1
    assert L.s4p_icp_rank_batch(arr, 64, order) == 0 and list(order)[:64] == list(range(64))
    with pytest.raises(icp_lib.ICPError):
        icp_lib.rank_batch([])
    # without a context the device entry points refuse before they touch anything
    T = np.tile(np.eye(4), (2, 1, 1))
    assert L.s4p_icp_refine_batch(None, None, 2, T.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), arr, order) == -1
    assert L.s4p_icp_sums_batch(None, 0, 2, None, None) == -1


def test_python_argument_checks_need_no_device(icp_lib):
    from super4pcs_amd import multiscale
    P = np.zeros((4, 3), np.float32)
    I2 = np.tile(np.eye(4), (2, 1, 1))
    with pytest.raises(ValueError):
        icp_lib.refine_best(P, P, I2)                                           # max_distance is required
    for kw in (dict(metric="gicp"), dict(metric="color"), dict(metric="nope"), dict(target_normals=P), dict(normal_radius=1.0)):
        with pytest.raises(ValueError):
            icp_lib.refine_best(P, P, I2, max_distance=1.0, **kw)
    for bad in (np.tile(np.eye(4), (65, 1, 1)), np.zeros((0, 4, 4)), np.eye(3), np.zeros((2, 4, 3)), np.zeros((2, 2, 4, 4))):
        with pytest.raises(ValueError):
            icp_lib.refine_best(P, P, bad, max_distance=1.0)
    assert icp_lib._batch_transforms(np.eye(4), np.float64).shape == (1, 4, 4)
    assert icp_lib._batch_transforms([np.eye(4)] * 64, np.float32).dtype == np.float32
    for kw in (dict(loss="huber"), dict(metric="gicp"), dict(metric="color"), dict(reciprocal=True), dict(normal_angle=60.0),
               dict(T0=np.eye(4))):
        with pytest.raises(ValueError):
            multiscale.refine_multiscale(P, P, starts=I2, voxel_sizes=(0.1, 0), max_distance=1.0, **kw)
    with pytest.raises(ValueError):
        multiscale.refine_multiscale(P, P, starts=np.tile(np.eye(4), (65, 1, 1)), voxel_sizes=(0,), max_distance=1.0)


def _build_app(outdir, extra=()):
    return apps.build_app(outdir, "icp_batch_app", ("dl",), ("-g", "-Werror") + tuple(extra))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_top_poses_program(tmp_path, flags):
    exe = _build_app(tmp_path, flags)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "0 failures" and len(lines) >= 18 and all(ln.startswith("ok  ") for ln in lines[:-1])


def test_cli_icp_starts_flag_parses_and_bad_uses_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for bad in (["--icp", "10", "--icp-starts", "0"], ["--icp", "10", "--icp-starts", "65"], ["--icp", "10", "--icp-starts", "4x"],
                ["--icp", "10", "--icp-starts", ""], ["--icp-starts", "4"], ["--icp", "0", "--icp-starts", "4"],
                ["--icp", "10", "--icp-starts", "4", "--icp-loss", "huber"],
                ["--icp", "10", "--icp-starts", "4", "--icp-loss", "trimmed", "--icp-trim", "0.5"],
                ["--icp", "10", "--icp-starts", "4", "--icp-metric", "gicp"],
                ["--icp", "10", "--icp-starts", "4", "--icp-metric", "color"],
                ["--icp", "10", "--icp-starts", "4", "--icp-reciprocal"],
                ["--icp", "10", "--icp-starts", "4", "--icp-normal-angle", "60"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-starts" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (["--icp-starts", "1"], ["--icp-starts", "64"], ["--icp-starts", "4", "--icp-metric", "plane"],
                 ["--icp-starts", "4", "--icp-scales", "0.04,0"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "10"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)
