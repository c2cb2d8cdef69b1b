"""Test-side restatements of the plane segmentation contract (include/s4p_plane.h): tests/plane_cpu/plane_cpu.cpp through
ctypes (float residuals by std::fmaf, 16 threads over candidates), a second, independent statement in numpy float64 with a
Python-integer splitmix64 and mulhi (residuals and candidate planes in float64, the refit sums by np.cumsum in the header's
two-level order, a Jacobi of its own in Python floats), the distance of every residual from the inlier bound, and the clouds
the host and the GPU tests share.  Only numpy is used."""
import ctypes as C
import math

import numpy as np

from tests import cluster_helpers as CH
from tests import normals_helpers as NH
from tests import normals_suite as S

SUM_BLOCK = 128
GOLDEN, MASK64 = 0x9E3779B97F4A7C15, (1 << 64) - 1

bits = NH.bits


def build_cpu(outdir):
    L = S.build_restatement("plane_cpu/plane_cpu.cpp", outdir, "libplane_cpu")
    vp = C.c_void_p
    L.plane_cpu_segment.restype = None
    L.plane_cpu_segment.argtypes = [vp, vp, vp, C.c_int64, C.c_float, C.c_int32, C.c_uint64, C.c_int32, vp, vp, vp, vp, vp, vp, C.c_int32]
    return CPU(L)


class CPU:
    def __init__(self, L):
        self.L = L

    def segment(self, X, distance, trials=1024, seed=0, refine=1, exclude=None, threads=16, all_counts=False):
        """(plane (4,) float32, mask (n,) uint8, info) as super4pcs_amd.plane.Plane.segment returns them; with all_counts the
        info also holds "counts" (int32 per candidate, 0 for an invalid one) and "valid" (uint8 per candidate)."""
        p = S.cols(X)
        n = p[0].shape[0]
        ex = None if exclude is None else np.ascontiguousarray(np.asarray(exclude) != 0, dtype=np.uint8)
        pl = np.zeros(8, np.float32); ints = np.zeros(4, np.int64); mask = np.zeros(n, np.uint8)
        counts = np.zeros(trials, np.int32); valid = np.zeros(trials, np.uint8)
        self.L.plane_cpu_segment(*S.xyzn(p), float(distance), int(trials), int(seed) & MASK64, int(refine), S.ptr(ex), pl.ctypes.data,
                                 ints.ctypes.data, mask.ctypes.data, counts.ctypes.data, valid.ctypes.data, int(threads))
        info = {"centre": pl[4:7].copy(), "d_centred": pl[7], "inliers": int(ints[0]), "alive": int(ints[1]), "trial": int(ints[2]),
                "valid_trials": int(ints[3])}
        if all_counts:
            info["counts"] = counts; info["valid"] = valid
        return pl[:4].copy(), mask, info


def same(a, b):
    """Bit equality of two (plane, mask, info) triples: the plane, d_centred, the centre, trial, valid_trials, inliers, alive
    and the mask."""
    (pa, ma, ia), (pb, mb, ib) = a, b
    ma, mb = S.to_host(ma), S.to_host(mb)
    return (np.array_equal(bits(pa), bits(pb)) and np.array_equal(ma, mb) and
            np.array_equal(bits(np.float32(ia["d_centred"])), bits(np.float32(ib["d_centred"]))) and
            np.array_equal(bits(ia["centre"]), bits(ib["centre"])) and
            all(ia[k] == ib[k] for k in ("trial", "valid_trials", "inliers", "alive")))


# ---- the numpy float64 statement ---------------------------------------------------------------------------------------------------

def splitmix_element(seed, k):
    """Element k (from 0) of the splitmix64 stream started at state seed, in Python integers."""
    z = (seed + (k + 1) * GOLDEN) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def _sign_rule(v):
    a = np.abs(v)
    lead = v[0] if (a[0] >= a[1] and a[0] >= a[2]) else (v[1] if a[1] >= a[2] else v[2])
    return -v if lead < 0 else v


def _jacobi(A):
    """The library's cyclic Jacobi in Python floats: (diagonal, V)."""
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


def _ordered_sum(rows):
    """The header's two-level sum of the rows of a float64 matrix: blocks of SUM_BLOCK rows from zero in order (np.cumsum adds
    in order), then the block sums in order."""
    parts = np.array([np.cumsum(rows[b:b + SUM_BLOCK], axis=0)[-1] for b in range(0, len(rows), SUM_BLOCK)])
    return np.cumsum(parts, axis=0)[-1]


def numpy_segment(X, distance, trials=1024, seed=0, refine=1, exclude=None, chunk=128):
    """The contract in numpy float64.  Returns (plane, mask, info); info also holds "counts" (of every candidate, float64
    residuals), "valid" and "planes": the (n, d') of the winner and of every refit, for residual_gap."""
    X = np.asarray(X, np.float32)
    n = len(X)
    lo, hi = X.min(0), X.max(0)
    c = (np.float32(0.5) * lo + np.float32(0.5) * hi).astype(np.float32)
    alive = np.arange(n) if exclude is None else np.flatnonzero(np.asarray(exclude) == 0)
    m = len(alive)
    Xc = (X[alive] - c).astype(np.float32).astype(np.float64)
    dist = float(np.float32(distance))
    N = np.zeros((trials, 3), np.float32); D = np.zeros(trials, np.float32); valid = np.zeros(trials, np.uint8)
    for t in range(trials):
        p = [(splitmix_element(seed & MASK64, 3 * t + a) * m) >> 64 for a in range(3)]
        if m < 3 or len(set(p)) < 3:
            continue
        a, b, cc = Xc[p[0]], Xc[p[1]], Xc[p[2]]
        if not (np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(cc).all()):
            continue
        e1, e2 = b - a, cc - a
        w = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
        l2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        if not (l2 > 0.0 and np.isfinite(l2)):
            continue
        v = _sign_rule(w / np.sqrt(l2))
        N[t] = v.astype(np.float32); D[t] = np.float32(-((v[0] * a[0] + v[1] * a[1]) + v[2] * a[2])); valid[t] = 1
    counts = np.zeros(trials, np.int64)
    for t0 in range(0, trials, chunk):
        R = N[t0:t0 + chunk].astype(np.float64) @ Xc.T + D[t0:t0 + chunk].astype(np.float64)[:, None]
        counts[t0:t0 + chunk] = (np.abs(R) <= dist).sum(1) * valid[t0:t0 + chunk]
    info = {"centre": c, "d_centred": np.float32(0), "inliers": 0, "alive": m, "trial": -1, "valid_trials": int(valid.sum()), "counts": counts,
            "valid": valid, "planes": []}
    mask = np.zeros(n, np.uint8)
    if not valid.any():
        return np.zeros(4, np.float32), mask, info
    win = int(np.flatnonzero(valid)[np.argmax(counts[valid != 0])])          # argmax returns the first largest
    nn, dd = N[win].copy(), D[win]

    def inl():
        return np.abs(Xc @ nn.astype(np.float64) + float(dd)) <= dist
    info["planes"].append((nn.copy(), dd))
    cur = inl()
    for _ in range(refine):
        k = int(cur.sum())
        if k < 3:
            break
        P = Xc[cur]
        S = _ordered_sum(np.concatenate([P, P[:, :1] * P, P[:, 1:2] * P[:, 1:], P[:, 2:] * P[:, 2:]], axis=1))
        mean = S[:3] / float(k)
        Cm = np.zeros((3, 3))
        idx = {(0, 0): 3, (0, 1): 4, (0, 2): 5, (1, 1): 6, (1, 2): 7, (2, 2): 8}
        for (i, j), s in idx.items():
            Cm[i, j] = Cm[j, i] = S[s] / float(k) - mean[i] * mean[j]
        if not ((Cm[0, 0] + Cm[1, 1]) + Cm[2, 2] > 0.0):
            break
        ev, V = _jacobi(Cm)
        best = 0
        for a in (1, 2):
            if ev[a] < ev[best]:
                best = a
        v = np.array([V[0][best], V[1][best], V[2][best]])
        v = _sign_rule(v / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        nn = v.astype(np.float32); dd = np.float32(-((v[0] * mean[0] + v[1] * mean[1]) + v[2] * mean[2]))
        info["planes"].append((nn.copy(), dd))
        cur = inl()
    mask[alive[cur]] = 1
    c64, n64 = c.astype(np.float64), nn.astype(np.float64)
    d = np.float32(float(dd) - ((n64[0] * c64[0] + n64[1] * c64[1]) + n64[2] * c64[2]))
    info.update(d_centred=dd, inliers=int(cur.sum()), trial=win)
    return np.array([nn[0], nn[1], nn[2], d], np.float32), mask, info


def residual_gap(X, distance, planes, exclude=None):
    """The smallest | |r| / distance - 1 | over all (plane, alive point) pairs, r in float64 on the centred float coordinates:
    how far the cloud stays from the inlier bound of the winning and the refit planes (numpy_segment's info["planes"])."""
    X = np.asarray(X, np.float32)
    c = (np.float32(0.5) * X.min(0) + np.float32(0.5) * X.max(0)).astype(np.float32)
    alive = np.arange(len(X)) if exclude is None else np.flatnonzero(np.asarray(exclude) == 0)
    Xc = (X[alive] - c).astype(np.float32).astype(np.float64)
    dist = float(np.float32(distance))
    return min(float(np.abs(np.abs(Xc @ nn.astype(np.float64) + float(dd)) / dist - 1.0).min()) for nn, dd in planes)


# ---- the clouds --------------------------------------------------------------------------------------------------------------------

TINY_N = (3, 4, 63, 64, 65, 255, 256, 257)
TILE = 4096                       # the points one workgroup pass of k_plane_count covers
BATCH = 128                       # one candidate batch
EDGE_N = TINY_N + (TILE - 1, TILE, TILE + 1)
EDGE_TRIALS = (1, 2, 63, 64, 65, BATCH - 1, BATCH, BATCH + 1)
TINY_DISTANCE = 0.05


def tiny_cloud(n, seed=1):
    """Three fifths of the points near the plane z = 0.3 x - 0.2 y + 0.1 (noise 0.01), the others uniform in the cube, permuted."""
    rng = np.random.default_rng(seed + 17 * n)
    P = rng.uniform(-1, 1, size=(n, 3))
    on = rng.permutation(n)[:max(3, (3 * n) // 5)]
    P[on, 2] = 0.3 * P[on, 0] - 0.2 * P[on, 1] + 0.1 + 0.01 * rng.normal(size=len(on))
    return P.astype(np.float32)


def duplicates_cloud(n=300, distinct=5, seed=3):
    """n points that are copies of `distinct` positions: most candidates draw two copies of one position and are invalid."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, size=(distinct, 3)).astype(np.float32)
    return base[rng.integers(0, distinct, n)]


def identical_cloud(n=100):
    return np.tile(np.array([[0.5, -1.25, 2.0]], np.float32), (n, 1))


def collinear_cloud(n=100, seed=4):
    """Integer multiples of (1, 2, -3) around the origin, permuted: every cross product is exactly zero."""
    k = np.random.default_rng(seed).permutation(n).astype(np.float32) - np.float32(n // 2)
    return np.stack([k, 2 * k, -3 * k], 1).astype(np.float32)


def lattice_cloud(side=8, seed=6):
    """side^3 integer points, permuted: at distance 0 and at distance 1 many candidates tie and residuals sit on the bound."""
    g = np.arange(side, dtype=np.float32)
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(P[np.random.default_rng(seed).permutation(len(P))])


def box_corner(seed=9, counts=(3000, 2000, 1200), extra=300):
    """Three faces of a box corner with unequal point counts (z = 0, x = 0, y = 0; noise 0.002) and a few points inside."""
    rng = np.random.default_rng(seed)
    parts = []
    for axis, k in enumerate(counts):
        F = rng.uniform(0.05, 1, size=(k, 3))
        F[:, (2, 0, 1)[axis]] = 0.002 * rng.normal(size=k)
        parts.append(F)
    parts.append(rng.uniform(0.2, 1, size=(extra, 3)))
    P = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(P[rng.permutation(len(P))])


lidar_cloud = CH.lidar_cloud
LIDAR = dict(distance=0.15, trials=1024, refine=1)


def large_cloud():
    """cluster_helpers.large_cloud() (524 289 points on the unit sphere) with every fifth point moved onto a planted disc
    z = 0.3 + 0.1 x of radius 0.9 (noise 0.002): above 128 x 4096 points a lane of k_plane_count takes a second
    trip, and the disc's count passes 2^16."""
    X = CH.large_cloud().copy()
    rng = np.random.default_rng(21)
    idx = np.arange(0, len(X), 5)
    r = 0.9 * np.sqrt(rng.uniform(0, 1, len(idx))); a = rng.uniform(0, 2 * np.pi, len(idx))
    x, y = r * np.cos(a), r * np.sin(a)
    X[idx] = np.stack([x, y, 0.3 + 0.1 * x + 0.002 * rng.normal(size=len(idx))], 1).astype(np.float32)
    return X
