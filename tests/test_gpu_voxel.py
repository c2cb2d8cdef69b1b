"""Voxel-grid downsampling on the device (include/s4p_voxel.h, super4pcs_amd/voxel.py) against the restatement of its
contract (tests/voxel_cpu, tests/voxel_helpers.py): out_xyz, out_attr, out_count, voxel_of and m bit for bit, through the
host entry point (numpy) and the device one (torch), at the block edges of the two-level sum and on the long-run path."""
import numpy as np
import pytest

from tests import normals_suite as S
from tests import voxel_helpers as VH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vox():
    return S.normals_module("voxel")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return VH.build_cpu(tmp_path_factory.mktemp("voxel_cpu"))


@pytest.fixture(scope="module")
def ctx(vox):
    c = vox.VoxelGrid(0)
    yield c
    c.close()


def _torch_args(X, A):
    return S.to_device(X), None if A is None else S.to_device(A)


@pytest.mark.parametrize("name", list(VH.CASES))
def test_downsample_equals_the_restatement_bit_for_bit(ctx, cpu, name):
    X, v, A = VH.CASES[name]()
    want = cpu.downsample(X, v, A)
    print("%s: n %d, m %d, largest voxel %d" % (name, len(X), len(want[0]), want[2].max() if len(want[2]) else 0))
    got = ctx.downsample(X, v, A)
    VH.assert_same(got, want, name + " (numpy)")
    assert isinstance(got[0], np.ndarray)
    Xt, At = _torch_args(X, A)
    got_t = ctx.downsample(Xt, v, At)
    assert got_t[0].is_cuda and got_t[3].is_cuda
    VH.assert_same(got_t, want, name + " (torch)")
    VH.assert_same(ctx.downsample(X, v, A), want, name + " (second call)")        # determinism across calls
    if name == "all_nonfinite":
        assert len(got[0]) == 0 and (got[3] == -1).all()
    if name == "tiny_voxel":
        assert len(got[0]) == len(X)
    if name == "nonfinite":
        assert np.isnan(got[1]).any() and (got[3] == -1).sum() == (~np.isfinite(X).all(1)).sum()


def test_extent_of_2_to_21_is_accepted_and_one_more_refused(vox, ctx, cpu):
    for axis in range(3):
        X = np.zeros((3, 3), np.float32)
        X[1, axis] = VH.MAX_EXTENT - 1
        X[2, axis] = 5.0
        VH.assert_same(ctx.downsample(X, 1.0), cpu.downsample(X, 1.0), "extent 2^21 on axis %d" % axis)
        X[1, axis] = VH.MAX_EXTENT
        with pytest.raises(VH.ExtentError):
            cpu.downsample(X, 1.0)
        with pytest.raises(vox.NormalsError) as e:
            ctx.downsample(X, 1.0)
        assert e.value.code == -1 and "%s axis" % "xyz"[axis] in str(e.value) and str(VH.MAX_EXTENT + 1) in str(e.value), str(e.value)
        with pytest.raises(vox.NormalsError) as e:
            ctx.downsample(S.to_device(X), 1.0)
        assert e.value.code == -1
    # a non-finite point does not count towards the extent
    X = np.array([[0, 0, 0], [np.inf, 0, 0], [1e30, np.nan, 0]], np.float32)
    got = ctx.downsample(X, 1.0)
    assert len(got[0]) == 1 and got[3].tolist() == [0, -1, -1]


def test_bad_arguments_are_refused(vox, ctx):
    import ctypes as C
    L = ctx.L
    X = np.random.default_rng(1).uniform(size=(10, 3)).astype(np.float32)
    cols = [np.ascontiguousarray(X[:, a]) for a in range(3)]
    px, py, pz = [c.ctypes.data for c in cols]
    A = np.zeros((10, 9), np.float32)
    out = np.zeros((10, 3), np.float32); oa = np.zeros((10, 9), np.float32); m = C.c_int64(7)
    po, pa, poa = out.ctypes.data, A.ctypes.data, oa.ctypes.data
    bad = {
        "n = 0": (px, py, pz, 0, 0.1, None, 0, po, None, None, None, C.byref(m)),
        "n < 0": (px, py, pz, -1, 0.1, None, 0, po, None, None, None, C.byref(m)),
        "n > 2^31 - 2": (px, py, pz, 2 ** 31 - 1, 0.1, None, 0, po, None, None, None, C.byref(m)),
        "voxel 0": (px, py, pz, 10, 0.0, None, 0, po, None, None, None, C.byref(m)),
        "voxel < 0": (px, py, pz, 10, -0.1, None, 0, po, None, None, None, C.byref(m)),
        "voxel nan": (px, py, pz, 10, float("nan"), None, 0, po, None, None, None, C.byref(m)),
        "voxel inf": (px, py, pz, 10, float("inf"), None, 0, po, None, None, None, C.byref(m)),
        "nattr 9": (px, py, pz, 10, 0.1, pa, 9, po, poa, None, None, C.byref(m)),
        "nattr -1": (px, py, pz, 10, 0.1, pa, -1, po, poa, None, None, C.byref(m)),
        "attr without nattr": (px, py, pz, 10, 0.1, pa, 0, po, None, None, None, C.byref(m)),
        "nattr without attr": (px, py, pz, 10, 0.1, None, 2, po, poa, None, None, C.byref(m)),
        "nattr without out_attr": (px, py, pz, 10, 0.1, pa, 2, po, None, None, None, C.byref(m)),
        "null x": (None, py, pz, 10, 0.1, None, 0, po, None, None, None, C.byref(m)),
        "null out_xyz": (px, py, pz, 10, 0.1, None, 0, None, None, None, None, C.byref(m)),
        "null m_out": (px, py, pz, 10, 0.1, None, 0, po, None, None, None, None),
    }
    for what, args in bad.items():
        for fn in (L.s4p_voxel_downsample, L.s4p_voxel_downsample_device):     # refused before any pointer is read
            assert fn(ctx.h, *args) == -1, what
            assert "voxel_downsample" in L.s4p_normals_last_error(ctx.h).decode(), what
    assert L.s4p_voxel_downsample(None, px, py, pz, 10, 0.1, None, 0, po, None, None, None, C.byref(m)) == -1
    # the optional outputs may be null
    assert L.s4p_voxel_downsample(ctx.h, px, py, pz, 10, 0.1, None, 0, po, None, None, None, C.byref(m)) == 0 and 1 <= m.value <= 10
    with pytest.raises(ValueError):
        ctx.downsample(X, 0.1, attrs=np.zeros((9, 1), np.float32))
    with pytest.raises(ValueError):
        ctx.downsample(X, 0.1, attrs=np.zeros((10, 9), np.float32))


def test_lidar_scene_at_a_multi_trip_size_equals_the_restatement_on_all_rows(vox, ctx, cpu):
    """524 289 points (one more than 2048 x 256: every grid-stride kernel takes a second trip) of the lidar scene with three
    channels, at a voxel size that keeps about a tenth of them, and with every point in one voxel (the long-run path with
    8193 blocks); numpy and torch."""
    import torch
    from super4pcs_amd import datasets as D
    n = 524_289
    X = np.ascontiguousarray(D.lidar_pair_scaled(0.12, delta=0.05)[0][:n], np.float32)
    assert len(X) == n
    A = VH.attrs_for(n, 3, 9)
    for v in (0.08, 4096.0):
        want = cpu.downsample(X, v, A)
        print("lidar %d at %g: m %d, largest voxel %d" % (n, v, len(want[0]), want[2].max()))
        VH.assert_same(ctx.downsample(X, v, A), want, "lidar numpy %g" % v)
        VH.assert_same(ctx.downsample(S.to_device(X), v, S.to_device(A)), want, "lidar torch %g" % v)
    assert want[2].max() > 64 * 64


def test_estimate_bits_are_unchanged_around_a_downsample(vox):
    from super4pcs_amd import datasets as D
    X = D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0]
    ctx = vox.VoxelGrid(0)
    try:
        ctx.set_cloud(X)
        before = ctx.estimate(16)
        Y, v, A = VH.one_voxel(4097, 8)
        ctx.downsample(Y, v, A)
        ctx.downsample(X, 0.01)
        after = ctx.estimate(16)
        assert np.array_equal(VH.bits(before), VH.bits(after)) and before.any()
    finally:
        ctx.close()


def test_one_shot_call_carries_attributes_and_renormalised_normals(vox, cpu):
    import torch
    from super4pcs_amd import datasets as D
    X = D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0]
    rng = np.random.default_rng(3)
    N = rng.normal(size=(len(X), 3)).astype(np.float32)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    N[:50] = 0                                            # "no normal" members pull the mean, an all-zero voxel stays zero
    rgb = rng.integers(0, 256, size=(len(X), 3)).astype(np.float32)
    v = 0.02
    wx, wa, wc, wv = cpu.downsample(X, v, np.concatenate([rgb, N], axis=1))
    d = wa[:, 3:].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nn = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        wn = (d / nn[:, None]).astype(np.float32)
    wn[~(nn > 0)] = 0
    xyz, a, nrm, cnt, vof = vox.voxel_downsample(X, v, attrs=rgb, normals=N)
    VH.assert_same((xyz, a, cnt, vof), (wx, wa[:, :3], wc, wv), "one-shot numpy")
    assert np.array_equal(VH.bits(nrm), VH.bits(wn))
    assert np.allclose(np.linalg.norm(nrm[nrm.any(1)], axis=1), 1, atol=1e-6)
    t = vox.voxel_downsample(S.to_device(X), v, attrs=S.to_device(rgb), normals=S.to_device(N))
    assert all(q.is_cuda for q in t)
    VH.assert_same((t[0], t[1], t[3], t[4]), (wx, wa[:, :3], wc, wv), "one-shot torch")
    assert np.array_equal(VH.bits(S.to_host(t[2])), VH.bits(wn))
    # one (n,) channel comes back as (m,); nothing asked for, nothing returned
    one = vox.voxel_downsample(X, v, attrs=rgb[:, 0])
    assert one[1].shape == (len(wx),) and one[2] is None and np.array_equal(VH.bits(one[1]), VH.bits(wa[:, 0]))
    none = vox.voxel_downsample(X, v)
    assert none[1] is None and none[2] is None and np.array_equal(VH.bits(none[0]), VH.bits(wx))


def test_facade_application_gives_the_python_rows_and_carries_normals_and_colours(vox, tmp_path):
    from tests import normals_helpers as NH
    X, v, _ = VH.CASES["duplicates"]()
    rng = np.random.default_rng(21)
    raw = rng.normal(size=(len(X), 3)).astype(np.float32)
    N = NH.point3d_normalise(raw)                         # what Point3D::set_normal stores of the file's values
    rgb = rng.integers(0, 256, size=(len(X), 3)).astype(np.float32)
    exe = S.build_facade_app(tmp_path)
    for mode, attrs, table in (("plain", None, X), ("attrs", np.concatenate([N, rgb], axis=1), np.concatenate([X, raw, rgb], axis=1))):
        xyz, a, _, _, vof = vox.voxel_downsample(X, v, attrs=attrs)
        heads, (got_vof,), rows = S.run_points_app(exe, ["voxel", "%.9g" % v, mode], table)
        m = len(xyz)
        assert heads == ["m %d" % m] and 1 < m < len(X)
        assert np.array_equal(got_vof, vof)
        rows = rows.astype(np.float32)
        assert rows.shape == (m, 9) and np.array_equal(VH.bits(rows[:, :3]), VH.bits(xyz))
        if attrs is None:
            assert not rows[:, 3:6].any() and (rows[:, 6:] == -1).all()                  # no normal, no colour
        else:
            assert np.array_equal(VH.bits(rows[:, 3:6]), VH.bits(NH.point3d_normalise(a[:, :3])))
            assert np.array_equal(VH.bits(rows[:, 6:]), VH.bits(a[:, 3:]))


def test_cli_voxel_size_matches_the_python_path(vox, s4p_lib_built, tmp_path):
    from tests import helpers as H
    P, Q, _ = H.small_pair(8000, delta=0.01, seed=33)
    # the Python path: downsample both clouds, then register with the same options; -r: the downsampled Q, registered: m rows
    Pv, Qv = S.cli_filter_equals_python(tmp_path, P, Q, ["--voxel-size", "0.03"], lambda Z: vox.voxel_downsample(Z, 0.03)[0], "Voxel grid: edge")
    assert 200 < len(Pv) < len(P) and 200 < len(Qv) < len(Q)
