"""The parts of libsuper4pcs_normals.so that several entry points share, on the MI355X.  The one neighbour walk: the normals
of estimate equal the restatement's normals of exactly the lists search returns (a cloud with duplicates and a lattice, so
that ties are broken by index), and the query forms equal the self forms.  The one arena: a context whose calls need more
and less work memory in turn returns what a fresh context returns, bit for bit, with numpy clouds and with GPU tensors;
contexts on one point and on one workgroup plus one lane equal the restatements."""
import numpy as np
import pytest

from tests import cluster_helpers as CH
from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S
from tests import orient_helpers as OH

pytestmark = pytest.mark.gpu
STEP = np.float32(0.125)                       # the lattice step: exact in binary, so d2 == fl(r * r) between lattice neighbours
VIEW = (0.3, -0.2, 2.0)


@pytest.fixture(scope="module")
def clu():
    S.normals_module("voxel").load_library()
    return S.normals_module("cluster")


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return NH.build_cpu(tmp_path_factory.mktemp("shared_normals_cpu"))


@pytest.fixture(scope="module")
def cluster_cpu(tmp_path_factory):
    return CH.build_cpu(tmp_path_factory.mktemp("shared_cluster_cpu"))


def walk_cloud():
    """300 points: a 5 x 5 x 5 lattice block, 135 random points around it, and 40 exact copies of points of both."""
    rng = np.random.default_rng(41)
    g = np.arange(5, dtype=np.float32) * STEP
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    loose = rng.uniform(-0.25, 0.75, size=(135, 3)).astype(np.float32)
    base = np.concatenate([lattice, loose])
    X = np.concatenate([base, base[rng.integers(0, len(base), 40)]]).astype(np.float32)
    return np.ascontiguousarray(X[rng.permutation(len(X))])


@pytest.fixture(scope="module")
def walk(clu):
    X = walk_cloud()
    assert X.shape == (300, 3) and len(np.unique(X, axis=0)) < 300
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    yield X, ctx
    ctx.close()


@pytest.mark.parametrize("radius", [None, STEP])
@pytest.mark.parametrize("k", [3, 8, 9, 16, 17, 32])
def test_estimate_and_search_walk_the_same_neighbours(walk, cpu, k, radius):
    X, ctx = walk
    idx, d2, cnt = ctx.search(k, radius, exclude_self=False)
    got = ctx.estimate(k, radius)
    want = cpu.normals_of_lists(X, idx)
    bad = np.flatnonzero((NH.bits(got) != NH.bits(want)).any(1))
    assert len(bad) == 0, (k, radius, len(bad), bad[:5], got[bad[:3]], want[bad[:3]], idx[bad[:3]])
    # the lists are what the test means them to be: ties by index, the radius bounds, zero normals below three neighbours
    tie = (d2[:, 1:] == d2[:, :-1]) & (idx[:, 1:] >= 0)
    assert tie.any() and (idx[:, 1:][tie] > idx[:, :-1][tie]).all()
    assert (cnt == (idx >= 0).sum(1)).all() and (cnt < k).any() == (radius is not None)
    assert (got[cnt < 3] == 0).all() and ((cnt < 3).any() == (radius is not None))
    at = ctx.estimate_at(X, k, radius)
    assert np.array_equal(NH.bits(at), NH.bits(got)), (k, radius)
    ai, ad, ac = ctx.search_at(X, k, radius)
    assert np.array_equal(ai, idx) and np.array_equal(KH.bits(ad), KH.bits(d2)) and np.array_equal(ac, cnt), (k, radius)


def _flat(out):
    """Every array of a call's result as bytes, every other value as it is."""
    if isinstance(out, (tuple, list)):
        return [_flat(v) for v in out]
    if isinstance(out, dict):
        return {key: _flat(v) for key, v in sorted(out.items())}
    if type(out).__module__.startswith("torch"):
        out = S.to_host(out)
    if isinstance(out, np.ndarray):
        return (out.dtype.str, out.shape, np.ascontiguousarray(out).tobytes())
    return out


def _sequence(wrap, tensors):
    """The cloud and (name, call on a context) in an order along which the work memory a call needs goes up and down."""
    from super4pcs_amd import voxel
    rng = np.random.default_rng(5)
    X = rng.uniform(0, 1, size=(1000, 3)).astype(np.float32)
    N0 = OH.random_normals(1000, 3)
    Q1 = (X[:1] + np.float32(0.01)).astype(np.float32)
    Q0 = np.zeros((0, 3), np.float32)
    V257 = rng.uniform(-1, 1, size=(257, 3)).astype(np.float32)
    V5000 = rng.uniform(-1, 1, size=(5000, 3)).astype(np.float32)      # the inner 0.7-voxels hold some 200 points each: long runs
    Xw, N0w, Q1w, Q0w, V257w, V5000w = (wrap(a) for a in (X, N0, Q1, Q0, V257, V5000))
    calls = [("dbscan", lambda c: c.dbscan(0.12, 4)),
             ("orient_towards", lambda c: c.orient_towards(N0w, VIEW)),
             ("search_at m=1", lambda c: c.search_at(Q1w, 8)),
             ("search k=32", lambda c: c.search(32)),
             ("estimate_at m=0", lambda c: c.estimate_at(Q0w, 8)),
             ("estimate_at m=1", lambda c: c.estimate_at(Q1w, 8)),
             ("statistical_outliers", lambda c: c.statistical_outliers(8, 1.5)),
             ("voxel 257", lambda c: voxel.VoxelGrid.downsample(c, V257w, 0.25)),
             ("voxel 5000", lambda c: voxel.VoxelGrid.downsample(c, V5000w, 0.7)),
             ("radius_outliers", lambda c: c.radius_outliers(0.15, 3)),
             # device_out only says on which device the result is allocated; the tensor itself is not written
             ("estimate", lambda c: c.estimate(16, None, device_out=Xw if tensors else None)),
             ("density", lambda c: c.density(0.12))]
    return Xw, calls


@pytest.mark.parametrize("form", ["numpy", "torch"])
def test_one_context_through_growing_and_shrinking_needs_equals_fresh_contexts(clu, form):
    if form == "torch":
        import torch
        X, calls = _sequence(S.to_device, True)
    else:
        X, calls = _sequence(np.asarray, False)
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    got = {}
    for name, call in calls:
        got[name] = _flat(call(ctx))
        fresh = clu.Cluster(0)
        fresh.set_cloud(X)
        want = _flat(call(fresh))
        fresh.close()
        assert got[name] == want, (form, name)
    ctx.close()
    assert np.frombuffer(got["voxel 5000"][2][2], np.int32).max() > 64          # the runs of more than one block were there
    assert got["estimate_at m=0"] == ("<f4", (0, 3), b"")


@pytest.mark.parametrize("n", [1, 257])
def test_one_point_and_one_workgroup_plus_one_lane_equal_the_restatements(clu, cpu, cluster_cpu, n):
    X = KH.tiny_cloud(n, False)
    N = OH.random_normals(n, 11 + n)
    eps = CH.tiny_eps(n)
    ctx = clu.Cluster(0)
    ctx.set_cloud(X)
    assert np.array_equal(NH.bits(ctx.estimate(3)), NH.bits(cpu.normals(X, 3))), n
    gi, gd, gc = ctx.search(1)
    wi, wd, wc = KH.numpy_lists(X, 1)
    assert np.array_equal(gi, wi) and np.array_equal(KH.bits(gd), KH.bits(wd)) and np.array_equal(gc, wc), n
    assert np.array_equal(ctx.density(eps), cluster_cpu.density(X, eps)), n
    label, kind, stats = ctx.dbscan(eps, 1)
    want_l, want_k, want_s = cluster_cpu.dbscan(X, eps, 1)
    assert np.array_equal(label, want_l) and np.array_equal(kind, want_k) and stats == want_s, (n, stats, want_s)
    out, info = ctx.orient(N, 8, None, None, return_info=True)
    idx = KH.numpy_lists(X, 8, None, exclude_self=True)[0]
    flip, comp, ncomp = OH.reference(X, N, idx, None)
    assert np.array_equal(info["flipped"], flip) and np.array_equal(info["component"], comp), n
    assert np.array_equal(OH.bits(out), OH.bits(OH.apply(N, flip))), n
    assert (info["vertices"], info["components"], info["flipped_count"]) == (int(OH.usable(N).sum()), ncomp, int(flip.sum())), (n, info)
    ctx.close()


@pytest.mark.parametrize("form", ["numpy", "torch"])
def test_calls_without_their_optional_outputs_equal_the_full_calls(clu, form):
    """The arena pieces that exist only when an optional output is asked for (cnt, mean_dist, flipped, component, out_count,
    voxel_of): the call without them returns, in what remains, the bits of the call with them.  Where the binding always
    passes the output (search, search_at, voxel_downsample), the C entry point is called as the binding calls it, with a null."""
    import ctypes as C
    from super4pcs_amd import _binding as B, voxel
    if form == "torch":
        import torch
        wrap, dev = S.to_device, True
    else:
        wrap, dev = np.asarray, False
    rng = np.random.default_rng(7)
    X = rng.uniform(0, 1, size=(1000, 3)).astype(np.float32)
    Q = rng.uniform(0, 1, size=(70, 3)).astype(np.float32)
    V = rng.uniform(-1, 1, size=(5000, 3)).astype(np.float32)
    Xw, Qw, Vw, Nw = wrap(X), wrap(Q), wrap(V), wrap(OH.random_normals(1000, 3))
    like = Xw if dev else None
    ctx = clu.Cluster(0)
    ctx.set_cloud(Xw)

    idx, d2, _ = ctx.search(8, 0.1)
    gi, pi = B.empty(like, (1000, 8), np.int32)
    gd, pd = B.empty(like, (1000, 8), np.float32)
    ctx._call("s4p_knn_search", like, 8, 0.1, 0, pi, pd, None)
    assert _flat([gi, gd]) == _flat([idx, d2])

    idx, d2, _ = ctx.search_at(Qw, 8, 0.1)
    _, ptr, m, keep = B.cols(Qw)
    gi, pi = B.empty(like, (m, 8), np.int32)
    gd, pd = B.empty(like, (m, 8), np.float32)
    ctx._call("s4p_knn_search_at", like, ptr[0], ptr[1], ptr[2], m, 8, 0.1, pi, pd, None)
    assert _flat([gi, gd]) == _flat([idx, d2])

    full = ctx.statistical_outliers(8, 1.5)
    bare = ctx.statistical_outliers(8, 1.5, want_mean_dist=False)
    assert bare[2] is None and _flat(bare[:2]) == _flat(full[:2])

    for viewpoint in (None, VIEW):
        out, _ = ctx.orient(Nw, 8, None, viewpoint, return_info=True)
        assert _flat(ctx.orient(Nw, 8, None, viewpoint)) == _flat(out), viewpoint

    xyz, _, _, _ = voxel.VoxelGrid.downsample(ctx, Vw, 0.7)
    _, ptr, n, keep = B.cols(Vw)
    gx, px = B.empty(like, (n, 3), np.float32)
    m = C.c_int64(0)
    ctx._call("s4p_voxel_downsample", like, ptr[0], ptr[1], ptr[2], n, 0.7, None, 0, px, None, None, None, C.byref(m))
    assert int(m.value) == len(xyz) and _flat(gx[:len(xyz)]) == _flat(xyz)
    del keep
    ctx.close()
