"""Plane segmentation on the MI355X (include/s4p_plane.h): the plane, d_centred, the centre, trial, valid_trials, inliers,
alive and the mask equal the restatement (tests/plane_cpu through tests/plane_helpers.py) bit for bit: at the edges of the
wave, the workgroup pass (4096 points) and the candidate batch (128 records), on clouds where most or all candidates are
invalid, on a lattice where counts tie and residuals sit on the bound, with an exclude mask, over three refit counts, on the
lidar cloud at the origin and at 1e4, and on 524 289 points where a lane takes further trips; peeling on a box corner; the
lidar pair through Python, the facade and the command line; determinism, numpy against torch, every refusal, and the
context's other calls after a plane call."""
import ctypes as C

import numpy as np
import pytest

from tests import apps
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import plane_helpers as PH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pln():
    return S.normals_module("plane")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return PH.build_cpu(tmp_path_factory.mktemp("plane_cpu"))


def _same(ctx, cpu, X, what, distance, trials=1024, seed=0, refine=1, exclude=None):
    """One segment call equals the restatement.  Returns the call's (plane, mask, info)."""
    got = ctx.segment(distance, trials, seed, refine, exclude)
    want = cpu.segment(X, distance, trials, seed, refine, exclude)
    assert got[0].dtype == np.float32 and got[0].shape == (4,) and got[1].dtype == np.uint8 and got[1].shape == (len(X),)
    print(what, got[0], got[2])
    assert PH.same(got, want), (what, got[0], want[0], got[2], want[2], int((got[1] != want[1]).sum()))
    assert got[2]["inliers"] == int(got[1].sum()) and set(np.unique(got[1]).tolist()) <= {0, 1}
    return got


@pytest.mark.parametrize("n", PH.EDGE_N)
def test_sizes_and_trials_at_the_edges_equal_the_restatement(pln, cpu, n):
    """n at the wave, at 256 and one below, at and above the 4096 points of a workgroup pass, crossed with trials one below, at
    and above the wave and the batch of 128 candidate records."""
    X = PH.tiny_cloud(n)
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    for trials in PH.EDGE_TRIALS:
        got = _same(ctx, cpu, X, (n, trials), PH.TINY_DISTANCE, trials, seed=n, refine=1)
        assert got[2]["alive"] == n and 0 <= got[2]["valid_trials"] <= trials
    ctx.close()


@pytest.mark.parametrize("refine", [0, 1, 3])
def test_refit_counts(pln, cpu, refine):
    X = PH.tiny_cloud(2049)
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    got = _same(ctx, cpu, X, ("refine", refine), PH.TINY_DISTANCE, 128, 5, refine)
    n = got[0][:3].astype(np.float64)
    assert abs(np.linalg.norm(n) - 1) < 1e-6 and np.abs(n).max() == n.max()          # unit, the largest component positive
    truth = np.array([-0.3, 0.2, 1.0]) / np.linalg.norm([-0.3, 0.2, 1.0])
    assert abs(n @ truth) > (0.999 if refine else 0.99) and got[2]["inliers"] > 1200
    ctx.close()


def test_duplicates_identical_and_collinear_clouds(pln, cpu):
    X = PH.duplicates_cloud(distinct=4)
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    got = _same(ctx, cpu, X, "duplicates", 0.01, 256, 0, 1)
    assert 0 < got[2]["valid_trials"] < 128 and got[2]["trial"] >= 0             # most candidates draw one position twice
    for X, what in ((PH.identical_cloud(), "identical"), (PH.collinear_cloud(), "collinear")):
        ctx.set_cloud(X)
        for refine in (0, 2):
            pl, mask, info = _same(ctx, cpu, X, what, 0.5, 200, 1, refine)
            assert info["trial"] == -1 and info["valid_trials"] == 0 and info["inliers"] == 0 and not mask.any() and not pl.any()
            assert info["alive"] == len(X) and info["d_centred"] == 0
    ctx.close()


@pytest.mark.parametrize("distance", [0.0, 1.0])
def test_lattice_ties_go_to_the_smallest_trial(pln, cpu, distance):
    """8^3 integer points: axis planes tie in count, and at distance 1 the neighbouring layers sit exactly on the bound."""
    X = PH.lattice_cloud()
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    pl, mask, info = _same(ctx, cpu, X, ("lattice", distance), distance, 256, 0, 0)
    counts = cpu.segment(X, distance, 256, 0, 0, all_counts=True)[2]["counts"]
    ties = np.flatnonzero(counts == counts.max())
    assert len(ties) > 1 and info["trial"] == ties[0] and info["inliers"] == counts.max() == (64 if distance == 0 else 192)
    ctx.close()


def test_exclude_equals_the_compacted_cloud(pln, cpu):
    X = PH.tiny_cloud(2049, seed=2)
    ex = (np.random.default_rng(3).uniform(size=len(X)) < 0.4).astype(np.uint8)
    ex[np.concatenate([X.argmin(0), X.argmax(0)])] = 0          # the points that span the bounds stay: the compacted cloud has the same frame
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    pl, mask, info = _same(ctx, cpu, X, "exclude", PH.TINY_DISTANCE, 130, 9, 1, ex)
    assert info["alive"] == int((ex == 0).sum()) and not mask[ex != 0].any() and info["inliers"] > 100
    # the same seed on the compacted cloud draws the same points: equal after scattering
    ctx.set_cloud(X[ex == 0])
    p2, m2, i2 = ctx.segment(PH.TINY_DISTANCE, 130, 9, 1)
    scattered = np.zeros(len(X), np.uint8)
    scattered[ex == 0] = m2
    assert np.array_equal(NH.bits(p2), NH.bits(pl)) and np.array_equal(scattered, mask)
    assert {k: v for k, v in i2.items() if k != "centre"} == {k: v for k, v in info.items() if k != "centre"}
    # two alive points: nothing to fit
    ctx.set_cloud(X)
    ex2 = np.ones(len(X), np.uint8)
    ex2[[5, 1000]] = 0
    pl, mask, info = _same(ctx, cpu, X, "two alive", PH.TINY_DISTANCE, 64, 0, 1, ex2)
    assert info["alive"] == 2 and info["trial"] == -1 and info["valid_trials"] == 0 and not mask.any()
    # bool masks are taken as they are
    assert PH.same(ctx.segment(PH.TINY_DISTANCE, 130, 9, 1, ex != 0), cpu.segment(X, PH.TINY_DISTANCE, 130, 9, 1, ex))
    ctx.close()


@pytest.mark.parametrize("shift", [0.0, 1.0e4])
def test_lidar_cloud_at_the_origin_and_far_from_it(pln, cpu, shift):
    X = (PH.lidar_cloud() + np.float32(shift)).astype(np.float32)
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    pl, mask, info = _same(ctx, cpu, X, ("lidar", shift), **PH.LIDAR)
    z = X[:, 2] - np.float32(shift)
    assert abs(pl[2]) > 0.999 and (np.abs(z[mask != 0]) < 0.15 + 0.01 * (shift > 0)).mean() >= 0.99 and mask[np.abs(z) < 0.1].mean() >= 0.99
    assert 11000 < info["inliers"] < 11800
    ctx.close()


def test_one_multi_trip_size_numpy_and_torch(pln, cpu):
    """524 289 points: above 128 x 4096 a lane of k_plane_count takes a second trip, above 2048 x 256 the lanes of
    the grid-stride kernels do, and the winner's count passes 2^16."""
    import torch
    X = PH.large_cloud()
    assert len(X) == 524_289
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    pl, mask, info = _same(ctx, cpu, X, "large", 0.01, 1024, 0, 1)
    assert info["inliers"] > 100_000 > 1 << 16 and abs(pl[2]) > 0.99
    assert PH.same(ctx.segment(0.01, 1024, 0, 1), (pl, mask, info))
    ctx.close()
    t = pln.Plane(0)
    t.set_cloud(S.to_device(X))
    pt, mt, it = t.segment(0.01, 1024, 0, 1)
    assert mt.is_cuda and mt.dtype == torch.uint8 and PH.same((pt, mt, it), (pl, mask, info))
    ex = S.to_device(mask)
    p2, m2, i2 = t.segment(0.01, 256, 1, 1, exclude=ex)
    assert PH.same((p2, m2, i2), cpu.segment(X, 0.01, 256, 1, 1, mask)) and i2["alive"] == len(X) - info["inliers"]
    t.close()


def test_segment_planes_on_a_box_corner(pln, cpu):
    X = PH.box_corner()
    planes, labels = pln.segment_planes(X, 0.01, max_planes=4, min_inliers=800, trials=512, seed=3)
    want_p, want_l = pln.peel_planes(lambda p, ex: cpu.segment(X, 0.01, 512, 3 + p, 1, ex), len(X), 4, 800)
    assert np.array_equal(NH.bits(planes), NH.bits(want_p)) and np.array_equal(labels, want_l) and labels.dtype == np.int32
    sizes = np.bincount(labels[labels >= 0]).tolist()
    assert len(planes) == 3 and sizes == sorted(sizes, reverse=True) and sizes[2] > 1100 and sizes[0] < 3300
    assert [int(np.argmax(np.abs(p[:3]))) for p in planes] == [2, 0, 1]                    # z = 0, x = 0, y = 0: descending size
    kept, keep, pl2 = pln.remove_planes(X, 0.01, count=2, trials=512, seed=3)
    assert np.array_equal(keep, (labels < 0) | (labels == 2))
    assert np.array_equal(kept, X[keep]) and np.array_equal(NH.bits(pl2), NH.bits(planes[:2]))


def test_lidar_pair_through_python_the_facade_and_the_command_line(pln, cpu, s4p_lib_built, tmp_path):
    from super4pcs_amd import datasets as D
    P, Q, _ = D.lidar_pair(20000)
    want = [cpu.segment(Z, 0.15, 1024, 0, 1) for Z in (P, Q)]
    removed = [w[2]["inliers"] for w in want]
    assert min(removed) > 5000
    for Z, w in zip((P, Q), want):
        kept, keep, planes = pln.remove_planes(Z, 0.15)
        assert np.array_equal(keep, w[1] == 0) and np.array_equal(kept, Z[keep]) and np.array_equal(NH.bits(planes[0]), NH.bits(w[0]))
    # the facade
    heads, (_, got_mask, _), rest = S.run_points_app(S.build_facade_app(tmp_path), ["plane", "0.15", "1024", "1", "1"], P)
    assert np.array_equal(NH.bits(np.array(heads[0].split()[1:], np.float32)), NH.bits(want[0][0]))
    assert heads[1] == "inliers %d" % removed[0] and np.array_equal(got_mask, want[0][1])
    assert heads[2:] == ["removed %d planes 1" % removed[0]]
    rest = rest.astype(np.float32)
    assert np.array_equal(NH.bits(rest[:, :3]), NH.bits(P[want[0][1] == 0])) and (rest[:, 3] == 1).all()
    assert np.array_equal(rest[:, 4].astype(np.int64), np.flatnonzero(want[0][1] == 0))
    # the command line: both inputs filtered, -r holds the kept points of the second
    apps.write_obj(tmp_path / "P.obj", P); apps.write_obj(tmp_path / "Q.obj", Q)
    M, out = apps.run_cli(S.cli(), tmp_path / "P.obj", tmp_path / "Q.obj", 0.05, 0.6, 200, ["--remove-plane", "0.15", "-r", tmp_path / "R.obj"])
    assert "removed %d of input1, %d of input2" % (removed[0], removed[1]) in out, out
    head, body = (tmp_path / "R.ply").read_bytes().split(b"end_header\n", 1)
    assert b"element vertex %d\n" % (len(Q) - removed[1]) in head and len(body) == 12 * (len(Q) - removed[1]) and np.isfinite(M).all()


def test_two_calls_and_both_forms_give_the_same_bits(pln):
    import torch
    X = PH.tiny_cloud(2049, seed=4)
    a = pln.segment_plane(X, PH.TINY_DISTANCE, 200, 7, 2)
    b = pln.segment_plane(X, PH.TINY_DISTANCE, 200, 7, 2)
    t = pln.segment_plane(S.to_device(X), PH.TINY_DISTANCE, 200, 7, 2)
    assert PH.same(a, b) and t[1].is_cuda and PH.same(a, t) and a[2]["trial"] >= 0
    assert not PH.same(a, pln.segment_plane(X, PH.TINY_DISTANCE, 200, 8, 0))           # another seed and no refit: another plane
    pt, lt = pln.segment_planes(S.to_device(X), PH.TINY_DISTANCE, 2, 100, 200, 7)
    pn, ln = pln.segment_planes(X, PH.TINY_DISTANCE, 2, 100, 200, 7)
    assert lt.is_cuda and lt.dtype == torch.int32 and np.array_equal(S.to_host(lt), ln) and np.array_equal(NH.bits(pt), NH.bits(pn))


def test_other_calls_on_the_context_are_unchanged_after_a_plane_call(pln):
    X = PH.lidar_cloud()
    ctx = pln.Plane(0)
    ctx.set_cloud(X)
    g0 = ctx.grid()
    n0 = ctx.estimate(16)
    i0, d0, c0 = ctx.search(8, exclude_self=True)
    l0, k0, s0 = ctx.dbscan(0.5, 10)
    ctx.segment(0.15)
    ctx.segment(0.15, 64, 1, 3, exclude=np.abs(X[:, 2]) < 0.15)
    assert ctx.grid() == g0
    assert np.array_equal(NH.bits(ctx.estimate(16)), NH.bits(n0))
    i1, d1, c1 = ctx.search(8, exclude_self=True)
    assert np.array_equal(i1, i0) and np.array_equal(NH.bits(d1), NH.bits(d0)) and np.array_equal(c1, c0)
    l1, k1, s1 = ctx.dbscan(0.5, 10)
    assert np.array_equal(l1, l0) and np.array_equal(k1, k0) and s1 == s0
    ctx.close()


def test_refusals(pln):
    X = np.random.default_rng(1).uniform(size=(100, 3)).astype(np.float32)
    ctx = pln.Plane(0)
    L, h = pln.load_library(), ctx.h
    mask = np.full(100, 7, np.uint8)
    res = pln.PlaneResult()
    opt = pln.PlaneOptions(0.1, 64, 0, 1)
    for fn in (L.s4p_plane_segment, L.s4p_plane_segment_device):
        assert fn(h, C.byref(opt), None, C.byref(res), mask.ctypes.data) == -7 and b"set_cloud first" in L.s4p_normals_last_error(h)
    ctx.set_cloud(X)
    nan, inf = float("nan"), float("inf")
    bad = [lambda: ctx.segment(nan), lambda: ctx.segment(inf), lambda: ctx.segment(-0.1), lambda: ctx.segment(0.1, trials=0),
           lambda: ctx.segment(0.1, trials=-4), lambda: ctx.segment(0.1, trials=(1 << 20) + 1), lambda: ctx.segment(0.1, refine=-1),
           lambda: ctx.segment(0.1, refine=17)]
    for i, call in enumerate(bad):
        with pytest.raises(pln.NormalsError) as e:
            call()
        assert e.value.code == -1 and len(str(e.value)) > 30, i
    for fn in (L.s4p_plane_segment, L.s4p_plane_segment_device):
        for args in ((None, None, C.byref(res), mask.ctypes.data), (C.byref(opt), None, None, mask.ctypes.data), (C.byref(opt), None, C.byref(res), None)):
            assert fn(h, *args) == -1 and len(L.s4p_normals_last_error(h)) > 20
        assert fn(None, C.byref(opt), None, C.byref(res), mask.ctypes.data) == -1
    assert (mask == 7).all()
    with pytest.raises(ValueError):
        ctx.segment(0.1, exclude=np.zeros(99, np.uint8))
    # the limits themselves are allowed: distance 0, one trial, 2^20 trials, sixteen refits
    assert ctx.segment(0.0, 1, 0, 0)[2]["valid_trials"] in (0, 1)
    assert ctx.segment(0.1, 1 << 20, 0, 16)[2]["valid_trials"] > 1 << 19
    ctx.close()
