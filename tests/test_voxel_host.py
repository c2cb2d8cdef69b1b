"""Voxel-grid downsampling and multi-scale ICP on the host: the header's declarations against the binding and the exports,
the new kernels in the library's namespace, the loud failure without a device, the restatement against a plain Python
dictionary implementation on the tiny shapes of the GPU tests, a crafted voxel on which the order of the sum shows,
refine_multiscale's argument checks, the command line's new flag and the facade header with and without Eigen."""
import re
import subprocess

import numpy as np
import pytest

from tests import normals_suite as S
from tests import voxel_helpers as VH


@pytest.fixture(scope="module")
def voxel():
    return S.normals_module("voxel")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return VH.build_cpu(tmp_path_factory.mktemp("voxel_cpu"))


def test_header_declarations_equal_the_binding_and_the_exports(voxel):
    from super4pcs_amd import knn, normals
    L = voxel.load_library()
    _, decl, exported = S.check_header("s4p_voxel.h", "s4p_voxel_", voxel.SYMBOLS, L, closed_prefixes="s4p_(?:normals|knn|outliers)_")
    assert len(decl) == 2
    for s in decl:
        assert len(getattr(L, s).argtypes) == 13, s
    # nothing new under the older prefixes
    assert sorted(set(re.findall(r"\b(s4p_normals_\w+)", exported))) == sorted(normals.SYMBOLS)
    assert sorted(set(re.findall(r"\b(s4p_(?:knn|outliers)_\w+)", exported))) == sorted(knn.SYMBOLS)


def test_new_kernels_live_in_the_library_namespace(voxel):
    from super4pcs_amd import normals
    S.check_kernels_in_namespace(["k_voxel_bounds", "k_voxel_keys", "k_voxel_heads", "k_voxel_runs", "k_voxel_segs", "k_voxel_long"] +
                                 ["k_voxel_%s<%d>" % (which, na) for na in range(9) for which in ("reduce", "partials")],
                                 stray=r"(?<!s4p_nrm::)\bk_voxel_\w+")
    needed = subprocess.run(["readelf", "-d", normals.LIB_PATH], capture_output=True, text=True).stdout
    libs = re.findall(r"NEEDED.*\[(.*?)\]", needed)
    assert any("amdhip64" in l for l in libs) and not [l for l in libs if re.search(r"rocblas|rocsolver|hipblas|torch|rccl", l)], libs


@pytest.mark.skipif(S.gpu_visible(), reason="checks the failure without a device")
def test_calls_fail_loudly_without_a_device(voxel):
    from super4pcs_amd import icp, multiscale
    X = np.zeros((10, 3), np.float32)
    S.check_no_device(voxel.NormalsError, (lambda: voxel.VoxelGrid(0), lambda: voxel.voxel_downsample(X, 0.1)))
    S.check_no_device((voxel.NormalsError, icp.ICPError), (lambda: multiscale.refine_multiscale(X, X, voxel_sizes=(0.1, 0), max_distance=0.1),))


@pytest.mark.parametrize("name", VH.TINY)
def test_restatement_equals_the_dictionary_implementation_on_the_tiny_shapes(cpu, name):
    X, v, A = VH.CASES[name]()
    want = VH.dict_downsample(X, v, A)
    got = cpu.downsample(X, v, A)
    VH.assert_same(got, want, name)
    m = len(got[0])
    assert got[2].sum() == np.isfinite(X).all(1).sum() and (np.unique(got[3][got[3] >= 0]) == np.arange(m)).all()
    if m > 1:                                             # rows ascend in (iz, iy, ix)
        v32 = float(np.float32(v))
        first = np.array([np.flatnonzero(got[3] == r)[0] for r in range(m)])
        idx = np.floor(X[first].astype(np.float64) / v32)[:, ::-1]
        assert all(tuple(idx[r]) < tuple(idx[r + 1]) for r in range(m - 1))


def test_lattice_points_floor_and_do_not_truncate(cpu):
    X = np.array([[-0.25, 0, 0], [-0.1, 0, 0], [-0.0, 0, 0], [0.1, 0, 0], [0.25, 0, 0], [np.nextafter(np.float32(-0.25), np.float32(-1)), 0, 0]],
                 np.float32)
    xyz, _, cnt, vof = cpu.downsample(X, 0.25)
    assert vof.tolist() == [1, 1, 2, 2, 3, 0] and cnt.tolist() == [1, 2, 2, 1]


def test_the_two_level_sum_differs_from_the_sequential_sum_and_from_numpy(cpu):
    """The crafted voxel (VH.crafted_values, seed VH.CRAFTED_SEED, 200 members of mixed magnitude that cancel): the
    contract's mean differs in bits from the plain sequential mean and from numpy's pairwise one, so a device path that
    summed in another order would not pass the GPU comparison.  The same for the shared one-voxel cases above one block,
    except 65 members: there the second block is one value, and the two orders are the same additions."""
    vals = VH.crafted_values()
    c = len(vals)
    X = np.full((c, 3), 0.5, np.float32)
    _, a, cnt, _ = cpu.downsample(X, 1.0, vals.reshape(-1, 1))
    assert cnt.tolist() == [c]
    d = [float(t) for t in vals]
    two, seq, pair = (np.float32(s / c) for s in (VH.two_level(d), VH.sequential(d), np.sum(vals.astype(np.float64))))
    print("crafted: two-level %.9g sequential %.9g numpy %.9g" % (two, seq, pair))
    assert VH.bits(a[0, 0]) == VH.bits(two)
    assert VH.bits(two) != VH.bits(seq) and VH.bits(two) != VH.bits(pair)
    for c in (65, 128, 129, 4097):
        X, v, A = VH.one_voxel(c, 3)
        _, a, cnt, vof = cpu.downsample(X, v, A)
        r = int(np.argmax(cnt))
        assert cnt[r] == c
        d = [float(t) for t in A[vof == r, 0]]
        assert VH.bits(a[r, 0]) == VH.bits(np.float32(VH.two_level(d) / c))
        assert (VH.bits(a[r, 0]) != VH.bits(np.float32(VH.sequential(d) / c))) == (c != 65), c


def test_renormalise():
    from super4pcs_amd import voxel
    N = np.array([[3, 0, 4], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-30, 0, 0], [0, -2, 0]], np.float32)
    out = voxel.renormalise(N)
    assert out.dtype == np.float32
    assert np.array_equal(out, np.array([[0.6, 0, 0.8], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, -1, 0]], np.float32))


def test_refine_multiscale_argument_checks():
    from super4pcs_amd import multiscale as M
    assert M.level_plan((0.04, 0.01, 0), max_distance=0.008) == [(0.04, 0.12, 30), (0.01, 0.03, 30), (0.0, 0.008, 30)]
    assert M.level_plan((0.04, None), max_distances=(0.1, 0.02), max_iterations=(5, 7)) == [(0.04, 0.1, 5), (0.0, 0.02, 7)]
    assert M.level_plan((0.04, 0.04, 0, 0), max_distance=1.0, max_iterations=4)[3] == (0.0, 1.0, 4)
    X = np.zeros((10, 3), np.float32)
    bad = [dict(voxel_sizes=(0.01, 0.04), max_distance=0.1),                    # increasing
           dict(voxel_sizes=(0, 0.04), max_distance=0.1),                       # 0 counts as smallest
           dict(voxel_sizes=(None, 0.04), max_distance=0.1),
           dict(voxel_sizes=(0.04, 0), max_distances=(0.1,)),                   # length mismatches
           dict(voxel_sizes=(0.04, 0), max_distance=0.1, max_iterations=(5, 5, 5)),
           dict(voxel_sizes=(0.04, 0)),                                         # no distance at all
           dict(voxel_sizes=(0.04, 0), max_distances=(0.1, 0.1), max_distance=0.1),
           dict(voxel_sizes=(), max_distance=0.1), dict(voxel_sizes=(-1.0,), max_distance=0.1),
           dict(voxel_sizes=(float("nan"),), max_distance=0.1), dict(voxel_sizes=0.1, max_distance=0.1),
           dict(voxel_sizes=(0,), max_distance=0.1, metric="nope"),
           dict(voxel_sizes=(0,), max_distance=0.1, metric="color", loss="huber")]
    for kw in bad:
        with pytest.raises(ValueError):
            M.refine_multiscale(X, X, **kw)


def test_cli_voxel_size_flag(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--voxel-size", "0"], ["--voxel-size", "-1"], ["--voxel-size", "x"], ["--voxel-size", ""], ["--voxel-size", "1x"],
             ["--voxel-size", "nan"], ["--voxel-size", "inf"], ["--voxel-size", "1e-60"], ["--voxel-size"]),
        good=(["--voxel-size", "0.5"], ["--voxel-size", "1e-3", "--remove-outliers", "16", "--estimate-normals", "16"],
              ["--icp", "5", "--voxel-size", "2"]),
        usage_word="--voxel-size", usage_order=("--remove-outliers k", "--voxel-size v"))


def test_cli_refuses_an_input_with_faces(tmp_path):
    S.check_cli_refuses_faces(tmp_path, ["--voxel-size", "0.2"])


@pytest.mark.parametrize("eigen", [False, True])
def test_facade_header_compiles_with_and_without_eigen(voxel, tmp_path, eigen):
    S.check_facade_header(tmp_path, "voxelgrid.h", eigen, "voxel", np.random.default_rng(2).uniform(size=(20, 3)),
                          no_device_args=["0.1", "plain"], no_device_text=("no HIP device",),
                          bad_args=(["0", "plain"], ["-1", "plain"], ["nan", "plain"], ["1e39", "plain"]), bad_text="VoxelDownsample:")


def test_cli_icp_scales_flag(tmp_path):
    S.check_cli_flags(
        tmp_path,
        bad=(["--icp-scales", "0.1"],                                        # needs --icp
             ["--icp", "0", "--icp-scales", "0.1"],
             ["--icp", "5", "--icp-scales", "0,0.1"],                         # only the last entry may be 0
             ["--icp", "5", "--icp-scales", "0.1,0.2"],                       # increasing
             ["--icp", "5", "--icp-scales", "x"], ["--icp", "5", "--icp-scales", ""], ["--icp", "5", "--icp-scales", "0.1,"],
             ["--icp", "5", "--icp-scales", ",0.1"], ["--icp", "5", "--icp-scales", "0.1,,0"], ["--icp", "5", "--icp-scales", "-1"],
             ["--icp", "5", "--icp-scales", "nan"], ["--icp", "5", "--icp-scales", "inf,1"], ["--icp", "5", "--icp-scales", "0.1x"],
             ["--icp", "5", "--icp-scales", "0.2 0.1"], ["--icp", "5", "--icp-scales", "1e-60"],
             ["--icp", "5", "--icp-scales", ",".join(["1"] * 17)], ["--icp", "5", "--icp-scales"]),
        good=(["--icp", "5", "--icp-scales", "0.2,0.1,0"], ["--icp-scales", "0.2", "--icp", "5"], ["--icp", "5", "--icp-scales", "0"],
              ["--icp", "5", "--icp-scales", "0.1,0.1"], ["--icp", "5", "--icp-scales", "4e-2,1e-2,0", "--icp-dist", "0.008"],
              ["--icp", "5", "--icp-scales", "0.2,0", "--icp-metric", "gicp", "--voxel-size", "0.01"],
              ["--icp", "5", "--icp-scales", ",".join(["1"] * 16)]),
        usage_word="--icp-scales", usage_order=("--voxel-size v", "--icp-scales v1"))


@pytest.mark.parametrize("eigen", [False, True])
def test_multiscale_facade_header_compiles_with_and_without_eigen(voxel, tmp_path, eigen):
    from super4pcs_amd import build as B
    from tests import multiscale_helpers as MH
    B.build_icp()
    exe = MH.build_app(tmp_path, S.check_header_alone(tmp_path, "icp_multiscale.h", eigen))
    pts = np.random.default_rng(2).uniform(size=(20, 3))
    VH.write_table(tmp_path / "P.xyz", pts); VH.write_table(tmp_path / "Q.xyz", pts); VH.write_table(tmp_path / "T0.txt", np.eye(4))
    args = [exe, str(tmp_path / "P.xyz"), str(tmp_path / "Q.xyz"), str(tmp_path / "T0.txt"), "point"]
    for bad in (["0.1:0.3:5", "0.2:0.6:5"], ["0:0.1:5", "0.1:0.3:5"], ["0.1:0:5"], ["-1:0.3:5"], ["nan:0.3:5"]):
        r = subprocess.run(args + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "RefineICPMultiScale:" in r.stderr, (bad, r.stderr)
    if not S.gpu_visible():
        r = subprocess.run(args + ["0.1:0.3:5", "0:0.1:5"], capture_output=True, text=True)
        assert r.returncode == 1 and "no HIP device" in r.stderr
