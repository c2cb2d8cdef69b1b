"""Test-side restatements of the radius-normals contract (include/s4p_shape.h): tests/shape_cpu/shape_cpu.cpp through ctypes (a
plain grid of edge 1.001 r or brute force, 16 threads over the queries), a second, independent statement in numpy with
Python integers for the moments, Python floats for the covariance and a Jacobi of its own (no numpy.linalg where bits are
compared), and the clouds the host and the GPU tests share.  scipy's k-d tree is used for the planted truth only, in float64,
where nothing is compared bit for bit."""
import ctypes as C
import functools
import math

import numpy as np

from tests import cluster_helpers as CH
from tests import normals_helpers as NH
from tests import normals_suite as S

U_BOUND = (1 << 19) + 1

bits = NH.bits


def build_cpu(outdir):
    L = S.build_restatement("shape_cpu/shape_cpu.cpp", outdir, "libshape_cpu")
    vp = C.c_void_p
    L.shape_cpu_estimate.restype = None
    L.shape_cpu_estimate.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, C.c_int64, C.c_float, C.c_int32, vp, vp, vp, vp, vp, C.c_int32, C.c_int32]
    return CPU(L)


class CPU:
    def __init__(self, L):
        self.L = L
        self.umax = 0                  # the largest |u| of any accepted neighbour over every call so far

    def estimate(self, X, radius, min_neighbours=3, queries=None, threads=16, brute=False, moments=False):
        """(normals (rows, 3) float32, eig (rows, 3) float32, count (rows,) int32) of the contract; with moments also an
        int64 (rows, 10) array: count, S0..S2, Qxx, Qxy, Qxz, Qyy, Qyz, Qzz."""
        p = S.cols(X)
        q = p if queries is None else S.cols(queries)
        m = q[0].shape[0]
        normals = np.empty((m, 3), np.float32); eig = np.empty((m, 3), np.float32); count = np.empty(m, np.int32)
        mom = np.empty((m, 10), np.int64) if moments else None
        top = np.zeros(1, np.int64)
        self.L.shape_cpu_estimate(*S.xyzn(p), *S.xyzn(q), float(radius), int(min_neighbours), normals.ctypes.data, eig.ctypes.data,
                                  count.ctypes.data, S.ptr(mom), top.ctypes.data, int(threads), int(bool(brute)))
        self.umax = max(self.umax, int(top[0]))
        return (normals, eig, count, mom) if moments else (normals, eig, count)


def same(a, b):
    """Bit equality of two (normals, eig, count) triples, each numpy or torch."""
    return all(x.shape == y.shape for x, y in zip(map(S.to_host, a[:3]), map(S.to_host, b[:3]))) and \
        np.array_equal(bits(S.to_host(a[0])), bits(S.to_host(b[0]))) and np.array_equal(bits(S.to_host(a[1])), bits(S.to_host(b[1]))) and \
        np.array_equal(S.to_host(a[2]), S.to_host(b[2]))


def differing(a, b):
    """How many rows differ in each of the three arrays: for a failing assertion's message."""
    return [int((bits(S.to_host(a[k])).reshape(len(S.to_host(a[2])), -1) != bits(S.to_host(b[k])).reshape(len(S.to_host(b[2])), -1)).any(1).sum())
            for k in (0, 1)] + [int((S.to_host(a[2]) != S.to_host(b[2])).sum())]


# ---- the numpy statement -------------------------------------------------------------------------------------------------------

def _jacobi(A):
    """The library's cyclic Jacobi in Python floats: (the three diagonal entries, V as rows)."""
    A = [[float(A[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    for _ in range(64):
        diag = (A[0][0] * A[0][0] + A[1][1] * A[1][1]) + A[2][2] * A[2][2]
        off = (A[0][1] * A[0][1] + A[0][2] * A[0][2]) + A[1][2] * A[1][2]
        if off == 0.0 or off <= 1e-36 * diag:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                if A[p][q] == 0.0:
                    continue
                theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q])
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(3):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq
                for k in range(3):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq
    return [A[0][0], A[1][1], A[2][2]], V


def scale_exponent(radius):
    """s = 18 - ilogb(r) of the float radius."""
    return 18 - (math.frexp(float(np.float32(radius)))[1] - 1)


def numpy_moments(X, radius, q):
    """(count, [S0, S1, S2], [Qxx, Qxy, Qxz, Qyy, Qyz, Qzz], the largest |u|) of one query position, in Python integers."""
    X = np.asarray(X, np.float32); q = np.asarray(q, np.float32)
    r = np.float32(radius)
    dx = X[:, 0] - q[0]; dy = X[:, 1] - q[1]; dz = X[:, 2] - q[2]
    d2 = dx * dx + (dy * dy + dz * dz)
    ok = d2 <= r * r
    factor = 2.0 ** scale_exponent(radius)
    u = [[int(v) for v in np.rint(e[ok].astype(np.float64) * factor)] for e in (dx, dy, dz)]
    cnt = int(ok.sum())
    S_ = [sum(u[a]) for a in range(3)]
    Q_ = [sum(x * y for x, y in zip(u[a], u[b])) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return cnt, S_, Q_, max([abs(v) for a in range(3) for v in u[a]], default=0)


def numpy_estimate(X, radius, min_neighbours=3, queries=None, want_moments=False):
    """The contract in numpy and Python numbers: (normals, eig, count), and with want_moments an int64 (rows, 10) array as
    CPU.estimate returns it.  Small clouds only: every point is tested for every query."""
    X = np.asarray(X, np.float32)
    Qs = X if queries is None else np.asarray(queries, np.float32)
    s = scale_exponent(radius)
    need = max(3, int(min_neighbours))
    N = np.zeros((len(Qs), 3), np.float32); E = np.zeros((len(Qs), 3), np.float32); cnts = np.zeros(len(Qs), np.int32)
    mom = np.zeros((len(Qs), 10), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, q in enumerate(Qs):
            if not np.isfinite(q).all():
                continue
            cnt, S_, Q_, top = numpy_moments(X, radius, q)
            assert top <= U_BOUND
            cnts[i] = cnt
            mom[i] = [cnt] + S_ + Q_
            if cnt < need:
                continue
            k = float(cnt)
            m = [float(S_[a]) / k for a in range(3)]
            idx = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}
            Cm = [[0.0] * 3 for _ in range(3)]
            for (a, b), t in idx.items():
                Cm[a][b] = Cm[b][a] = float(Q_[t]) / k - m[a] * m[b]
            if not ((Cm[0][0] + Cm[1][1]) + Cm[2][2] > 0.0):
                continue
            ev, V = _jacobi(Cm)
            best = 0
            for a in (1, 2):
                if ev[a] < ev[best]:
                    best = a
            v = [V[0][best], V[1][best], V[2][best]]
            ln = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            v = [x / ln for x in v]
            a0, a1, a2 = abs(v[0]), abs(v[1]), abs(v[2])
            lead = v[0] if (a0 >= a1 and a0 >= a2) else (v[1] if a1 >= a2 else v[2])
            if lead < 0.0:
                v = [-x for x in v]
            N[i] = [np.float32(x) for x in v]
            E[i] = [np.float32(math.ldexp(x, -2 * s)) for x in sorted(ev, reverse=True)]
    return (N, E, cnts, mom) if want_moments else (N, E, cnts)


def surface_variation(eig):
    eig = np.asarray(eig, np.float32)
    total = (eig[:, 0] + eig[:, 1]) + eig[:, 2]
    ok = total > 0
    return np.where(ok, eig[:, 2] / np.where(ok, total, np.float32(1)), np.float32(0)).astype(np.float32)


def angles_deg(A, B):
    """The angle between the lines along the rows of A and B, in degrees, float64."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64)
    c = np.abs((A * B).sum(1)) / np.maximum(np.linalg.norm(A, axis=1) * np.linalg.norm(B, axis=1), 1e-300)
    return np.degrees(np.arccos(np.clip(c, 0.0, 1.0)))


# ---- the clouds --------------------------------------------------------------------------------------------------------------------

SIZES = (1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 4097)
BEYOND = 2.0                         # beyond the extent of every unit-cube cloud: sqrt(3) < 2


def cube_cloud(n, seed=0):
    """n points uniform in the unit cube, a tenth of them (from n = 20) copies of earlier ones."""
    rng = np.random.default_rng(7000 + 13 * n + seed)
    P = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    if n >= 20:
        c = n // 10
        P[n - c:] = P[rng.integers(0, n - c, c)]
    return P


def cube_radius(n, neighbours=20):
    """The radius of a ball that holds about `neighbours` of n uniform points in the unit cube (at most 0.6)."""
    return np.float32(min(0.6, (neighbours / (n * 4.18879)) ** (1.0 / 3.0)))


def lattice_cloud(side=8, seed=6):
    g = np.arange(side, dtype=np.float32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(P[np.random.default_rng(seed).permutation(len(P))])


def below(x):
    """The float just below x."""
    return np.nextafter(np.float32(x), np.float32(0))


def identical_cloud(n=100):
    return np.tile(np.array([[0.5, -1.25, 2.0]], np.float32), (n, 1))


def collinear_cloud(n=100, seed=4):
    """Integer multiples of (1, 2, -3) x 1/64 around the origin, permuted: the covariance has rank one."""
    k = (np.random.default_rng(seed).permutation(n).astype(np.float32) - np.float32(n // 2)) / np.float32(64)
    return np.stack([k, 2 * k, -3 * k], 1).astype(np.float32)


def coplanar_cloud(n=400, seed=5):
    """Points of the plane z = 0.25 on a grid of step 1/64 (exact in float, so the smallest eigenvalue is an exact zero or a
    rounding residue of either sign, which the contract keeps)."""
    rng = np.random.default_rng(seed)
    P = np.zeros((n, 3), np.float32)
    P[:, :2] = rng.integers(0, 64, size=(n, 2)).astype(np.float32) / np.float32(64)
    P[:, 2] = 0.25
    return P


def two_far_clusters(n=600, seed=8, gap=4.0, spread=1.0e-3):
    """Two clusters of n / 2 points, `spread` wide and `gap` apart: at a radius of the spread's order the grid of edge r would
    have (gap / r)^3 cells, so it is enlarged and its 3 x 3 x 3 block is far wider than r."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(0, spread, size=(n, 3))
    P[n // 2:] += gap
    return np.ascontiguousarray(P[rng.permutation(n)].astype(np.float32))


def scale_cloud(n=300, seed=11):
    """n points uniform in [-2, 2]^3: scaled by 2^-40 its spacing stays above set_cloud's smallest cell edge."""
    return np.random.default_rng(seed).uniform(-2, 2, size=(n, 3)).astype(np.float32)


large_cloud = CH.large_cloud
LARGE_RADIUS = 0.012                 # about 19 neighbours on the unit sphere with 524 289 points


def moment_cloud(n=20000, seed=12):
    """n points in the unit cube: at the radius BEYOND every point is every point's neighbour and the sums of squares pass 2^32."""
    return np.random.default_rng(seed).uniform(0, 1, size=(n, 3)).astype(np.float32)


PLANTED = dict(n=300000, queries=3000, radius=0.02, truth_radius=0.01, knn=32, below_deg=5.0, above_deg=20.0)


@functools.lru_cache(maxsize=1)
def planted():
    """(Q, the 3000 query positions, their truth normals): Q is the second cloud of datasets.bumpy_pair(300000) with its
    default noise (sigma = delta = 0.004); the queries are 3000 seeded points of Q; the truth of a query is the
    smallest-eigenvalue direction of the noise-free cloud (noise_sigma = 0, same seed and motion, so point i of it is point i
    of Q without its noise) within 0.01 of the query's noise-free position, in float64."""
    from scipy.spatial import cKDTree
    from super4pcs_amd import datasets as D
    Q = D.bumpy_pair(PLANTED["n"])[1]
    Q0 = D.bumpy_pair(PLANTED["n"], noise_sigma=0.0)[1].astype(np.float64)
    pick = np.sort(np.random.default_rng(2024).choice(len(Q), PLANTED["queries"], replace=False))
    tree = cKDTree(Q0)
    truth = np.zeros((len(pick), 3))
    for t, nb in enumerate(tree.query_ball_point(Q0[pick], PLANTED["truth_radius"])):
        Z = Q0[nb] - Q0[nb].mean(0)
        truth[t] = np.linalg.eigh(Z.T @ Z)[1][:, 0]
    return Q, np.ascontiguousarray(Q[pick]), truth
