"""Test-side restatement of the clustering contract (include/s4p_cluster.h): tests/cluster_cpu/cluster_cpu.cpp through ctypes
(its own cell grid and union-find, 16 threads), a full-matrix numpy brute force for small clouds (d2 in float32 in the
contract's order, the border rule by lexsort on (d2 bits, index), labels ranked by the smallest core index), and the clouds
the host and the GPU tests share.  Only numpy is used: no scipy, no sklearn."""
import ctypes as C

import numpy as np

from tests import knn_helpers as KH
from tests import normals_helpers as NH
from tests import normals_suite as S

NOISE, BORDER, CORE = 0, 1, 2
STAT_KEYS = ("core", "border", "noise", "clusters")

bits = NH.bits


def build_cpu(outdir):
    L = S.build_restatement("cluster_cpu/cluster_cpu.cpp", outdir, "libcluster_cpu")
    vp = C.c_void_p
    L.cluster_cpu_dbscan.restype = None
    L.cluster_cpu_dbscan.argtypes = [vp, vp, vp, C.c_int64, C.c_float, C.c_int32, vp, vp, vp, C.c_int32]
    L.cluster_cpu_density.restype = None
    L.cluster_cpu_density.argtypes = [vp, vp, vp, C.c_int64, C.c_float, vp, C.c_int32]
    return CPU(L)


class CPU:
    def __init__(self, L):
        self.L = L

    def dbscan(self, X, eps, min_points, threads=16):
        """(label int32[n], kind uint8[n], stats dict) of the contract."""
        p = S.cols(X)
        n = p[0].shape[0]
        label = np.empty(n, np.int32); kind = np.empty(n, np.uint8); st = np.zeros(4, np.int64)
        self.L.cluster_cpu_dbscan(*S.xyzn(p), float(eps), int(min_points), label.ctypes.data, kind.ctypes.data, st.ctypes.data, int(threads))
        return label, kind, dict(zip(STAT_KEYS, (int(v) for v in st)))

    def density(self, X, radius, threads=16):
        p = S.cols(X)
        count = np.empty(p[0].shape[0], np.int32)
        self.L.cluster_cpu_density(*S.xyzn(p), float(radius), count.ctypes.data, int(threads))
        return count


def d2_matrix(X):
    """float32 (n, n): dx*dx + (dy*dy + dz*dz) with dx = fl(x_j - x_i)."""
    X = np.asarray(X, np.float32)
    dx = X[None, :, 0] - X[:, None, 0]; dy = X[None, :, 1] - X[:, None, 1]; dz = X[None, :, 2] - X[:, None, 2]
    return (dx * dx + (dy * dy + dz * dz)).astype(np.float32)


def numpy_dbscan(X, eps, min_points):
    """The contract from the full distance matrix: (label, kind, stats, count).  Small clouds only."""
    X = np.asarray(X, np.float32)
    n = len(X)
    D = d2_matrix(X)
    assert np.array_equal(bits(D), bits(D.T))                 # d2 is symmetric in its bits
    r2 = np.float32(eps) * np.float32(eps)
    A = D <= r2
    count = A.sum(1).astype(np.int32)
    core = count >= min_points
    # components of the core graph by spreading the smallest index until nothing moves
    comp = np.where(core, np.arange(n), n)
    G = A & core[None, :] & core[:, None]
    while True:
        new = np.where(core, np.where(G, comp[None, :], n).min(1, initial=n), n)
        new = np.minimum(new, comp)
        if np.array_equal(new, comp):
            break
        comp = new
    roots = np.unique(comp[core])                             # ascending smallest core index
    rank = {int(r): k for k, r in enumerate(roots)}
    label = np.full(n, -1, np.int32)
    kind = np.zeros(n, np.uint8)
    for i in range(n):
        if core[i]:
            label[i] = rank[int(comp[i])]; kind[i] = CORE
            continue
        js = np.flatnonzero(A[i] & core)
        if len(js):
            j = js[np.lexsort((js, bits(D[i, js])))[0]]
            label[i] = rank[int(comp[j])]; kind[i] = BORDER
    stats = {"core": int(core.sum()), "border": int((kind == BORDER).sum()), "noise": int((kind == NOISE).sum()), "clusters": len(roots)}
    return label, kind, stats, count


def sizes(label):
    """Cluster sizes, largest first."""
    label = np.asarray(label)
    return sorted(np.bincount(label[label >= 0]).tolist(), reverse=True) if (label >= 0).any() else []


# ---- the clouds ---------------------------------------------------------------------------------------------------------------

TINY_N = KH.TINY_N
TINY_MIN_POINTS = (1, 2, 4)


def tiny_eps(n):
    return np.float32(1.6) * KH.tiny_radius(n)


def border_tie(seed):
    """25 points on a line: four copies each at x in {-1, -0.5, 0, 2, 2.5, 3} and one point at x = 1, permuted.  At eps = 1,
    min_points = 10 the point at x = 1 has count 9 and eight core neighbours at d2 = 1, four in each of the two clusters.
    Returns (cloud, the index of the point at x = 1)."""
    xs = np.repeat(np.array([-1, -0.5, 0, 2, 2.5, 3], np.float32), 4)
    X = np.zeros((25, 3), np.float32)
    X[:24, 0] = xs
    X[24, 0] = 1
    perm = np.random.default_rng(seed).permutation(25)
    return np.ascontiguousarray(X[perm]), int(np.flatnonzero(perm == 24)[0])


BORDER_TIE_LEFT = (0, 4, 5)          # seeds where the smallest index among the eight lies at x = 0; 1, 2, 3: at x = 2


def chain(n=4096, seed=0):
    """n collinear points at integer x, permuted: the core graph at eps = 1 is a path of diameter n - 1."""
    X = np.zeros((n, 3), np.float32)
    X[:, 0] = np.random.default_rng(seed).permutation(n).astype(np.float32)
    return X


def lattice_of_ties(n=400, seed=8):
    """Integer coordinates x 0.25 with a tenth duplicated: many exactly equal distances, d2 == r2 at eps = 0.25."""
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 6, size=(n, 3)).astype(np.float32) * np.float32(0.25)
    P[n // 3:n // 3 + n // 10] = P[:n // 10]
    return P


def fragment_cloud():
    """The 6210-point cloud of DESIGN.md section 29: the bumpy surface, a dense 150-point blob at (1.2, 0, 0) and 60 planted
    points.  Returns (cloud, planted mask)."""
    from super4pcs_amd import datasets as D
    surface = D.bumpy_pair(6000, noise_sigma=0.001, seed=12)[0]
    blob = (np.array([1.2, 0, 0]) + 0.02 * np.random.default_rng(7).normal(size=(150, 3))).astype(np.float32)
    return KH.plant(np.concatenate([surface, blob]).astype(np.float32), 60)


FRAGMENT = dict(eps=0.03, min_points=4, n=6210, sizes=[6001, 149], stats={"core": 6150, "border": 0, "noise": 60, "clusters": 2}, removed=209)


def lidar_cloud():
    from super4pcs_amd import datasets as D
    return D.lidar_pair(20000)[0]


LIDAR = {(0.5, 10): dict(stats={"core": 9776, "border": 2341, "noise": 7883, "clusters": 83}, largest=10340),
         (0.3, 5): dict(stats={"core": 8343, "border": 2141, "noise": 9516, "clusters": 357}, largest=None)}


def large_cloud():
    """524 289 points on the unit sphere, those with |z| < 0.05 pushed 0.05 outwards in z: two caps and a few stragglers.
    Above 2048 x 256 points a lane of every grid-stride kernel takes a second and a third trip."""
    from super4pcs_amd import datasets as D
    X = D.sphere_cloud(524_289, 3).copy()
    band = np.abs(X[:, 2]) < 0.05
    X[band, 2] += np.where(X[band, 2] >= 0, np.float32(0.05), np.float32(-0.05))
    return X


LARGE = dict(eps=0.012, min_points=6, sizes=[262383, 261876, 6], stats={"core": 523355, "border": 910, "noise": 24, "clusters": 3})


def boundary_gap(X, eps, rows=500):
    """The smallest |dist / eps - 1| over all pairs, distances in double from the float coordinates, eps as the float the
    library gets: how far the cloud's pairs stay from the eps boundary.  Blocks of rows of the full matrix."""
    P = np.asarray(X, np.float32).astype(np.float64)
    e = float(np.float32(eps))
    sq = (P * P).sum(1)
    best = np.inf
    for a in range(0, len(P), rows):
        Q = P[a:a + rows]
        d = Q[:, None, :] - P[None, :, :] if len(P) <= 2000 else None
        if d is not None:
            D = (d * d).sum(2)
        else:
            D = np.maximum(sq[a:a + rows, None] + sq[None, :] - 2.0 * (Q @ P.T), 0.0)
            near = np.abs(np.sqrt(D) / e - 1.0) < 1e-3          # the expansion loses digits: redo the near ones exactly
            ii, jj = np.nonzero(near)
            dd = Q[ii] - P[jj]
            D = np.full(1, np.inf) if len(ii) == 0 else (dd * dd).sum(1)
        best = min(best, float(np.abs(np.sqrt(D) / e - 1.0).min()))
    return best
