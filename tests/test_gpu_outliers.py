"""Outlier removal on the MI355X (include/s4p_knn.h): the statistical filter's mean distances, mu, sigma, t and mask against
the CPU restatement with correctly rounded sums, its edge cases, the radius filter's mask against numpy, determinism,
numpy against torch, the facade application and the command line's --remove-outliers."""
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def knn():
    return S.normals_module("knn")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("knn_cpu"))


@pytest.fixture(scope="module")
def planted():
    from super4pcs_amd import datasets as D
    return {"bumpy": KH.plant(D.bumpy_pair(6000, overlap=0.5, delta=0.004, seed=12)[0], 60),
            "lidar": KH.plant(D.lidar_pair_scaled(0.004, delta=0.05)[0], 200)}


@pytest.fixture(scope="module")
def contexts(knn, planted):
    out = {}
    for name, (X, _) in planted.items():
        ctx = knn.Knn(0)
        ctx.set_cloud(X)
        out[name] = ctx
    yield out
    for ctx in out.values():
        ctx.close()


@pytest.fixture(scope="module")
def reference_lists(cpu, planted):
    """The restatement's 33 nearest of every point (itself included), once per cloud: every k's list without self is the
    first k of (these minus the own index)."""
    return {name: cpu.knn(X, 33, None, threads=16)[0] for name, (X, _) in planted.items()}


def _reference_m(X, idx33, k):
    fn = lambda X_, k_, r_, queries: (idx33[:, :k_].copy(), (idx33[:, :k_] >= 0).sum(1).astype(np.int32))      # noqa: E731
    _, d2, cnt = KH.lists(fn, X, k, None, None, True)
    assert (cnt == min(k, len(X) - 1)).all()
    return KH.mean_dist(d2, cnt)


@pytest.mark.parametrize("name,k,ratio", [("bumpy", 1, 2.0), ("bumpy", 8, 2.0), ("bumpy", 16, 2.0), ("bumpy", 32, 2.0),
                                          ("lidar", 16, 2.0), ("lidar", 8, 1.0)])
def test_statistical_removal_equals_the_reference(knn, planted, contexts, reference_lists, name, k, ratio):
    X, is_planted = planted[name]
    keep, stats, md = contexts[name].statistical_outliers(k, ratio)
    assert keep.dtype == bool and md.dtype == np.float64 and keep.shape == (len(X),) and md.shape == (len(X),)
    m_ref = _reference_m(X, reference_lists[name], k)
    KH.check_sor(len(X), k, ratio, md, stats, keep, m_ref, name)
    if name == "bumpy":                                  # the filter does its job: the surface stays, the strays go
        assert keep[~is_planted].all() and (~keep[is_planted]).sum() >= 51, (~keep[is_planted]).sum()


def test_statistical_removal_edge_cases(knn, cpu):
    ctx = knn.Knn(0)
    # n = 1: no neighbour, m = 0, sigma = 0, kept
    ctx.set_cloud(np.array([[1, 2, 3]], np.float32))
    keep, st, md = ctx.statistical_outliers(16, 2.0)
    assert keep.tolist() == [True] and md.tolist() == [0.0]
    assert st == {"n": 1, "mean": 0.0, "stddev": 0.0, "threshold": 0.0, "kept": 1}
    # n = 2: each is the other's only neighbour
    X = np.array([[0, 0, 0], [3, 4, 0]], np.float32)
    ctx.set_cloud(X)
    keep, st, md = ctx.statistical_outliers(16, 2.0)
    assert keep.tolist() == [True, True] and md.tolist() == [5.0, 5.0]
    assert st == {"n": 2, "mean": 5.0, "stddev": 0.0, "threshold": 5.0, "kept": 2}
    # 300 identical points: every m = 0, t = 0, all kept because 0 <= 0
    ctx.set_cloud(np.tile(np.array([[0.5, -0.25, 2.0]], np.float32), (300, 1)))
    keep, st, md = ctx.statistical_outliers(8, 2.0)
    assert keep.all() and not md.any() and st == {"n": 300, "mean": 0.0, "stddev": 0.0, "threshold": 0.0, "kept": 300}
    # k = 32 on 20 points: every list holds the 19 others
    X = np.random.default_rng(4).uniform(size=(20, 3)).astype(np.float32)
    ctx.set_cloud(X)
    for ratio in (0.0, 1.0):
        keep, st, md = ctx.statistical_outliers(32, ratio)
        _, d2, cnt = KH.numpy_lists(X, 32, exclude_self=True)
        assert (cnt == 19).all()
        KH.check_sor(20, 32, ratio, md, st, keep, KH.mean_dist(d2, cnt), "20 points")
    ctx.close()


def _numpy_radius_mask(X, r, mn):
    """At least mn other points with d2 <= fl(r * r): a count over the whole float32 distance matrix, in row blocks."""
    X = np.asarray(X, np.float32)
    r2 = np.float32(r) * np.float32(r)
    out = np.empty(len(X), bool)
    for lo in range(0, len(X), 1000):
        Q = X[lo:lo + 1000]
        dx = X[None, :, 0] - Q[:, None, 0]; dy = X[None, :, 1] - Q[:, None, 1]; dz = X[None, :, 2] - Q[:, None, 2]
        out[lo:lo + 1000] = ((dx * dx + (dy * dy + dz * dz)) <= r2).sum(1) - 1 >= mn
    return out


def test_radius_removal_equals_numpy(knn, planted, contexts):
    X, is_planted = planted["bumpy"]
    for r, mn in ((0.01, 1), (0.02, 8), (0.05, 32)):
        want = _numpy_radius_mask(X, r, mn)
        keep = contexts["bumpy"].radius_outliers(r, mn)
        assert keep.dtype == bool and np.array_equal(keep, want), (r, mn, np.flatnonzero(keep != want)[:5])
        print("radius %g, min %d: kept %d of %d, planted kept %d" % (r, mn, keep.sum(), len(X), keep[is_planted].sum()))
        assert 0 < keep.sum() < len(X)
    for n in KH.TINY_N:
        for dup in (False, True):
            Xs = KH.tiny_cloud(n, dup)
            ctx = knn.Knn(0)
            ctx.set_cloud(Xs)
            for mn in (1, 2, 8, 32):
                r = float(KH.tiny_radius(n)) * (1.0 if mn == 1 else 2.5)
                assert np.array_equal(ctx.radius_outliers(r, mn), _numpy_radius_mask(Xs, r, mn)), (n, dup, mn)
            ctx.close()


def test_two_calls_and_numpy_torch_agree(knn, planted, contexts):
    import torch
    X, _ = planted["lidar"]
    ctx = contexts["lidar"]
    k1, s1, m1 = ctx.statistical_outliers(16, 2.0)
    k2, s2, m2 = ctx.statistical_outliers(16, 2.0)
    assert np.array_equal(k1, k2) and np.array_equal(m1.view(np.uint64), m2.view(np.uint64))
    assert all(np.float64(s1[f]).view(np.uint64) == np.float64(s2[f]).view(np.uint64) for f in ("mean", "stddev", "threshold")) and s1 == s2
    r1 = ctx.radius_outliers(0.05, 8)
    assert np.array_equal(r1, ctx.radius_outliers(0.05, 8))
    # the one-shot functions, numpy and torch
    kept, mask, stats = knn.remove_statistical_outliers(X, k=16, std_ratio=2.0)
    assert isinstance(kept, np.ndarray) and np.array_equal(mask, k1) and stats == s1 and np.array_equal(kept, X[k1])
    Xt = S.to_device(X)
    kept_t, mask_t, stats_t = knn.remove_statistical_outliers(Xt, k=16, std_ratio=2.0)
    assert kept_t.is_cuda and mask_t.is_cuda and mask_t.dtype == torch.bool and stats_t == s1
    assert np.array_equal(S.to_host(mask_t), k1) and np.array_equal(S.to_host(kept_t), X[k1])
    tctx = knn.Knn(0)
    tctx.set_cloud(Xt)
    _, _, md_t = tctx.statistical_outliers(16, 2.0)
    assert md_t.is_cuda and md_t.dtype == torch.float64 and np.array_equal(S.to_host(md_t).view(np.uint64), m1.view(np.uint64))
    tctx.close()
    kept, mask = knn.remove_radius_outliers(X, 0.05, 8)
    kept_t, mask_t = knn.remove_radius_outliers(Xt, 0.05, 8)
    assert np.array_equal(mask, r1) and np.array_equal(S.to_host(mask_t), r1) and np.array_equal(S.to_host(kept_t), kept)
    assert np.array_equal(kept, X[r1])


def test_facade_application_gives_the_same_mask(knn, planted, contexts, tmp_path):
    X, _ = planted["bumpy"]
    exe = S.build_facade_app(tmp_path)
    np.savetxt(tmp_path / "P.xyz", X, fmt="%.9g")
    Xr = np.loadtxt(tmp_path / "P.xyz", dtype=np.float32)
    assert np.array_equal(Xr, X)
    for args, want in ((["stat", "16", "2.0"], contexts["bumpy"].statistical_outliers(16, 2.0)[0]),
                       (["radius", "0.02", "8"], contexts["bumpy"].radius_outliers(0.02, 8))):
        heads, (mask,), rest = S.run_points_app(exe, ["outliers"] + args, X)
        assert heads == ["removed %d" % (~want).sum()]
        assert len(mask) == len(X) and np.array_equal(mask.astype(bool), want)
        # erased in place, order kept, normals and colours moved with their points
        assert np.array_equal(rest[:, :3].astype(np.float32), X[want]) and (rest[:, 3] == 1.0).all()
        assert np.array_equal(rest[:, 4].astype(np.int64), np.flatnonzero(want))


def test_cli_remove_outliers_matches_the_python_path(knn, s4p_lib_built, tmp_path):
    P, Q, _ = H.small_pair(8000, delta=0.01, seed=33)
    P, _ = KH.plant(P, 40)
    Q, _ = KH.plant(Q, 40)
    # the Python path: filter both clouds, then register with the same options; -r: the filtered Q, registered
    Pk, Qk = S.cli_filter_equals_python(tmp_path, P, Q, ["--remove-outliers", "16"],
                                        lambda Z: knn.remove_statistical_outliers(Z, k=16, std_ratio=2.0)[0], "Removed outliers: k 16")
    assert 0 < len(P) - len(Pk) < 400 and 0 < len(Q) - len(Qk) < 400
    # an input with faces is refused
    KH.write_obj(tmp_path / "F.obj", Q[:100], faces=[(1, 2, 3)])
    r = subprocess.run([S.cli(), "-i", str(tmp_path / "P.obj"), str(tmp_path / "F.obj"), "--remove-outliers", "16"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 254 and "faces" in r.stdout + r.stderr
