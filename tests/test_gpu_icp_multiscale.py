"""Multi-scale ICP (super4pcs_amd/multiscale.py) on the device: refine_multiscale is, bit for bit, the hand-written chain of
voxel_downsample and icp.refine calls for every metric and a robust loss; a single level at voxel 0 is icp.refine; and the
basin: a start from which single-level ICP stays far from the truth and the coarse-to-fine chain does not."""
import numpy as np
import pytest

from tests import multiscale_helpers as MH

pytestmark = pytest.mark.gpu

VOXELS = (0.15, 0.06, 0)
D_FINE = 0.05
ITERATIONS = (12, 10, 8)

CONFIGS = {
    "point": dict(metric="point"),
    "plane, estimated normals": dict(metric="plane"),
    "plane, given normals": dict(metric="plane", target_normals="Np"),
    "gicp": dict(metric="gicp", target_normals="Np", source_normals="Nq"),
    "gicp, estimated normals": dict(metric="gicp"),
    "color": dict(metric="color", target_normals="Np", target_intensity="Ip", source_intensity="Iq"),
    "point, huber": dict(metric="point", loss="huber"),
    "plane, trimmed": dict(metric="plane", target_normals="Np", loss="trimmed", trim_fraction=0.8),
}


@pytest.fixture(scope="module")
def mods():
    from super4pcs_amd import build as B
    B.build_icp()
    B.build_normals()
    from super4pcs_amd import icp, multiscale, voxel
    return icp, multiscale, voxel


@pytest.fixture(scope="module")
def case():
    return MH.small_pair()


def _same_result(a, b):
    return bytes(a) == bytes(b)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_refine_multiscale_is_the_chain_of_downsample_and_refine(mods, case, name):
    icp, multiscale, voxel = mods
    cfg = dict(CONFIGS[name])
    metric = cfg.pop("metric")
    given = {k: case[cfg.pop(k)] for k in ("target_normals", "source_normals", "target_intensity", "source_intensity") if k in cfg}
    P, Q, T0 = case["P"], case["Q"], case["T0"]
    T, levels = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=VOXELS, max_distance=D_FINE, max_iterations=ITERATIONS, metric=metric,
                                             **given, **cfg)
    assert len(levels) == 3
    # the chain by hand
    Tc = T0
    for l, (v, it) in enumerate(zip(VOXELS, ITERATIONS)):
        d = max(D_FINE, 3.0 * v)
        if v > 0:
            Pl, Ipl, Npl, _, _ = voxel.voxel_downsample(P, v, attrs=given.get("target_intensity"), normals=given.get("target_normals"))
            Ql, Iql, Nql, _, _ = voxel.voxel_downsample(Q, v, attrs=given.get("source_intensity"), normals=given.get("source_normals"))
            assert 20 < len(Pl) < len(P) and 20 < len(Ql) < len(Q)
        else:
            Pl, Ql = P, Q
            Npl, Nql = given.get("target_normals"), given.get("source_normals")
            Ipl, Iql = given.get("target_intensity"), given.get("source_intensity")
        Tc, r = icp.refine(Pl, Ql, T0=Tc, max_distance=d, metric=metric, target_normals=Npl, source_normals=Nql, target_intensity=Ipl,
                           source_intensity=Iql, max_iterations=it, **cfg)
        assert _same_result(r, levels[l]), (name, l, r.as_dict(), levels[l].as_dict())
        assert r.n_corr > 0
    assert np.array_equal(T, Tc), name
    e0, e1 = MH.pose_error(T0, case["T_gt"], Q), MH.pose_error(T, case["T_gt"], Q)
    # printed, not asserted: on this half-overlapping pair the coarse levels' large distances pair points outside the overlap,
    # and the few fine iterations need not undo that; what this test pins is the composition
    print("%s: pose error %.4g -> %.4g, iterations %s" % (name, e0, e1, [r.iterations for r in levels]))


def test_explicit_distances_and_torch_inputs_give_the_same_chain(mods, case):
    import torch
    icp, multiscale, voxel = mods
    P, Q, T0 = case["P"], case["Q"], case["T0"]
    dists = [max(D_FINE, 3.0 * v) for v in VOXELS]
    a = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=VOXELS, max_distance=D_FINE, max_iterations=ITERATIONS)
    b = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=VOXELS, max_distances=dists, max_iterations=ITERATIONS)
    c = multiscale.refine_multiscale(torch.from_numpy(P).cuda(), torch.from_numpy(Q).cuda(), T0=T0, voxel_sizes=(0.15, 0.06, None),
                                     max_distance=D_FINE, max_iterations=ITERATIONS)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and all(_same_result(x, y) for x, y in zip(a[1], other[1]))


def test_a_single_level_at_voxel_0_is_refine(mods, case):
    icp, multiscale, voxel = mods
    P, Q, T0 = case["P"], case["Q"], case["T0"]
    for kw in (dict(metric="point"), dict(metric="plane", target_normals=case["Np"]), dict(metric="point", loss="tukey")):
        T, levels = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=(0,), max_distance=D_FINE, max_iterations=20, **kw)
        Tr, r = icp.refine(P, Q, T0=T0, max_distance=D_FINE, max_iterations=20, **kw)
        assert np.array_equal(T, Tr) and len(levels) == 1 and _same_result(levels[0], r)
    with pytest.raises(ValueError):                       # icp.refine's own refusals come through
        multiscale.refine_multiscale(P, Q, voxel_sizes=(0,), max_distance=D_FINE, metric="gicp", loss="huber")
    with pytest.raises(ValueError):
        multiscale.refine_multiscale(P, Q, voxel_sizes=(0.1, 0), max_distance=D_FINE, metric="point", target_intensity=case["Ip"],
                                     source_intensity=case["Iq"])


def test_coarse_to_fine_reaches_the_minimum_from_a_start_outside_the_single_level_basin(mods):
    """The reduced-scale lidar pair (100 000 returns per scan, known pose), d = 4 delta at the finest level.  From a start 20
    degrees off, single-level refine with the whole iteration budget (90) ends more than 10 x farther from the truth than it
    ends from a 1 degree start; refine_multiscale (voxels 0.4, 0.15, 0; 30 iterations each) from the same start ends within
    2 x of the from-1-degree result.  Measured (root mean square displacement of Q, metres): from 1 degree 0.00234; from 20
    degrees single-level 0.129, multi-scale 0.00198."""
    icp, multiscale, voxel = mods
    P, Q, T_gt = MH.basin_pair()
    total = MH.BASIN_ITERATIONS * len(MH.BASIN_VOXELS)
    T1, _ = icp.refine(P, Q, T0=MH.basin_start(T_gt, Q, 1.0), max_distance=MH.BASIN_D, max_iterations=total)
    T0 = MH.basin_start(T_gt, Q, MH.BASIN_START_DEG)
    Ts, _ = icp.refine(P, Q, T0=T0, max_distance=MH.BASIN_D, max_iterations=total)
    Tm, levels = multiscale.refine_multiscale(P, Q, T0=T0, voxel_sizes=MH.BASIN_VOXELS, max_distance=MH.BASIN_D,
                                              max_iterations=MH.BASIN_ITERATIONS)
    e1, es, em = (MH.pose_error(T, T_gt, Q) for T in (T1, Ts, Tm))
    print("basin: start %g deg (%.4f); from 1 deg %.5f; single-level %.5f; multi-scale %.5f, iterations %s" % (
        MH.BASIN_START_DEG, MH.pose_error(T0, T_gt, Q), e1, es, em, [r.iterations for r in levels]))
    assert es > 10 * e1                                   # the case stays meaningful
    assert em <= 2 * e1


APP_LEVELS = [(0.15, 0.45, 12), (0.06, 0.18, 10), (0.0, 0.05, 8)]


@pytest.mark.parametrize("metric", ["point", "plane", "huber"])
def test_facade_application_is_the_restated_chain_bit_for_bit(mods, case, tmp_path, metric):
    """RefineICPMultiScale (tests/icp_multiscale_app) against its order of operations restated on the Python binding
    (MH.facade_chain): the pose, every level's iterations, status, n_corr, rmse and fitness, and the moved Q, bit for bit.
    The facade moves Q's copy by the float pose on the host and refines from the identity, where refine_multiscale hands
    the double pose to icp.refine; the restatement follows the facade."""
    import subprocess
    icp, multiscale, voxel = mods
    P, Q, T0 = case["P"], case["Q"], case["T0"].astype(np.float32)
    exe = MH.build_app(tmp_path)
    np.savetxt(tmp_path / "P.xyz", P, fmt="%.9g"); np.savetxt(tmp_path / "Q.xyz", Q, fmt="%.9g")
    np.savetxt(tmp_path / "T0.txt", T0, fmt="%.9g")
    out = subprocess.run([exe, str(tmp_path / "P.xyz"), str(tmp_path / "Q.xyz"), str(tmp_path / "T0.txt"), metric] +
                         ["%.17g:%.17g:%d" % lv for lv in APP_LEVELS], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    lines = out.stdout.splitlines()
    got_T = np.array([float(t) for t in lines[0].split()[1:17]], np.float64).astype(np.float32).reshape(4, 4)
    kw = {"point": {}, "plane": dict(metric="plane"), "huber": dict(loss="huber")}[metric]
    T, results, Qm = MH.facade_chain(icp, voxel, P, Q, T0, APP_LEVELS, **kw)
    print("%s: pose error %.4g -> %.4g, iterations %s" % (metric, MH.pose_error(T0, case["T_gt"], Q), MH.pose_error(T, case["T_gt"], Q),
                                                          [r.iterations for r in results]))
    assert np.array_equal(got_T.view(np.uint32), T.view(np.uint32)), (got_T, T)
    for l, r in enumerate(results):
        it, status, n_corr, rmse, fitness = lines[1 + l].split()[1:]
        assert (int(it), int(status), int(n_corr)) == (r.iterations, r.status, r.n_corr), (l, lines[1 + l], r.as_dict())
        assert float(rmse) == r.rmse and float(fitness) == r.fitness, (l, lines[1 + l], r.as_dict())
        assert r.n_corr > 0
    moved = np.array([[float(t) for t in ln.split()] for ln in lines[1 + len(results):]], np.float64).astype(np.float32)
    assert np.array_equal(moved.view(np.uint32), Qm.view(np.uint32))
    assert not np.array_equal(T, T0)


def test_cli_icp_scales_matches_the_python_path(mods, s4p_lib_built, tmp_path):
    """`--icp 10 --icp-scales 0.06,0.02,0` against the Python path: register with capi.Matcher, then the restated chain with
    d_l = max(4 delta, 3 v_l) and 10 iterations per level.  The -r file holds binary floats and is compared bit for bit; the
    matrix file is text of limited precision, so it is compared within 2e-6, the bound tests/test_gpu_icp.py uses for the
    same file after --icp."""
    import subprocess
    from super4pcs_amd import build as B, capi
    from tests import helpers as H
    from tests import voxel_helpers as VH
    icp, multiscale, voxel = mods
    delta, overlap, n_s = 0.01, 0.6, 200
    P, Q, _ = H.small_pair(8000, delta=delta, seed=33)
    VH.write_obj(tmp_path / "P.obj", P); VH.write_obj(tmp_path / "Q.obj", Q)
    cli = B.build_cli()
    r = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "-o", str(overlap), "-d", str(delta), "-n", str(n_s),
                        "-t", "1000", "--icp", "10", "--icp-scales", "0.06,0.02,0", "-m", str(tmp_path / "mat.txt"),
                        "-r", str(tmp_path / "reg.obj")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (r.stdout + r.stderr).count("ICP level ") == 3
    got = np.array([[float(t) for t in ln.split()] for ln in (tmp_path / "mat.txt").read_text().splitlines()[2:6]])
    gm = capi.Matcher(capi.make_options(delta, overlap, n_s))
    _, M, _ = gm.compute_transformation(P, Q)
    levels = [(v, max(4.0 * delta, 3.0 * v), 10) for v in (0.06, 0.02, 0.0)]
    T, results, Qm = MH.facade_chain(icp, voxel, P, Q, np.asarray(M, np.float32), levels)
    print("cli:\n%s\npython:\n%s\niterations %s" % (got, T, [x.iterations for x in results]))
    assert np.max(np.abs(got - T.astype(np.float64))) <= 2e-6
    assert np.max(np.abs(T - np.asarray(M, np.float32))) > 0
    head, body = (tmp_path / "reg.ply").read_bytes().split(b"end_header\n", 1)
    assert b"element vertex %d\n" % len(Q) in head
    assert np.array_equal(np.frombuffer(body, "<f4").reshape(-1, 3).view(np.uint32), Qm.view(np.uint32))
