"""Test-side restatements of the descriptor contract (include/s4p_feature.h): tests/feature_cpu/feature_cpu.cpp through ctypes
(a plain grid of edge 1.001 r or brute force, 16 threads; a brute-force matcher), a second, independent statement in numpy
with float32 arrays for the pair features (numpy never contracts) and Python integers for H, S, A and D, with a boundary
table of its own from math.cos and math.sin, and the clouds, normals and the registration pair the host and the GPU tests
share."""
import ctypes as C
import functools
import math

import numpy as np

from tests import cluster_helpers as CH
from tests import normals_suite as S
from tests import shape_helpers as SH

BINS = 33
F32 = np.float32


def build_cpu(outdir):
    L = S.build_restatement("feature_cpu/feature_cpu.cpp", outdir, "libfeature_cpu")
    vp = C.c_void_p
    L.feature_cpu_fpfh.restype = None
    L.feature_cpu_fpfh.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_float, vp, vp, vp, C.c_int32, C.c_int32]
    L.feature_cpu_match.restype = C.c_int32
    L.feature_cpu_match.argtypes = [vp, C.c_int64, vp, C.c_int64, C.c_int32, vp, vp, C.c_int32]
    return CPU(L)


class CPU:
    def __init__(self, L):
        self.L = L

    def fpfh(self, X, N, radius, threads=16, brute=False, spfh=False):
        """(F (n, 33) uint16, count (n,) int32) of the contract; with spfh also the S rows (n, 33) uint16."""
        p = S.cols(X)
        n = p[0].shape[0]
        nrm = np.ascontiguousarray(N, np.float32)
        assert nrm.shape == (n, 3)
        F = np.empty((n, BINS), np.uint16); count = np.empty(n, np.int32)
        Srows = np.empty((n, BINS), np.uint16) if spfh else None
        self.L.feature_cpu_fpfh(*S.xyzn(p), nrm.ctypes.data, float(radius), F.ctypes.data, count.ctypes.data, S.ptr(Srows), int(threads), int(bool(brute)))
        return (F, count, Srows) if spfh else (F, count)

    def match(self, fa, fb, mutual=True, threads=16):
        """(idx (m,) int32, dist (m,) int32), or None when a value exceeds 4096."""
        fa = np.ascontiguousarray(fa, np.uint16).reshape(-1, BINS); fb = np.ascontiguousarray(fb, np.uint16).reshape(-1, BINS)
        idx = np.empty(len(fa), np.int32); dist = np.empty(len(fa), np.int32)
        rc = self.L.feature_cpu_match(fa.ctypes.data, len(fa), fb.ctypes.data, len(fb), 1 if mutual else 0, idx.ctypes.data, dist.ctypes.data, int(threads))
        return None if rc else (idx, dist)


def same(a, b):
    """Equality of two (F, count) pairs, each numpy or torch."""
    a = [S.to_host(x) for x in a[:2]]; b = [S.to_host(x) for x in b[:2]]
    return all(x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def differing(a, b):
    return [int((S.to_host(a[0]) != S.to_host(b[0])).any(1).sum()), int((S.to_host(a[1]) != S.to_host(b[1])).sum())]


def pairs_of(idx):
    """(k, 2) int32 of (a, idx[a]) over the rows with a partner: what features.match_features returns."""
    idx = np.asarray(S.to_host(idx))
    a = np.flatnonzero(idx >= 0)
    return np.stack([a, idx[a]], 1).astype(np.int32).reshape(-1, 2)


# ---- the numpy statement -------------------------------------------------------------------------------------------------------

def theta_bounds():
    """The ten boundary directions as floats, from math: ((fl(cos beta_k), fl(sin beta_k)), k = 1 .. 10)."""
    return [(F32(math.cos(-math.pi + 2 * math.pi * k / 11)), F32(math.sin(-math.pi + 2 * math.pi * k / 11))) for k in range(1, 11)]


def header_bounds():
    """The table as include/s4p_feature.h writes it."""
    import re
    txt = open(S.INCLUDE + "/s4p_feature.h").read()
    body = txt[txt.index("#define S4P_FEATURE_THETA_BOUNDS"):txt.index("#ifdef __cplusplus")]
    v = [F32(x) for x in re.findall(r"(-?\d\.\d+)f", body)]
    assert len(v) == 20
    return list(zip(v[0::2], v[1::2]))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _bin11(f):
    t = F32(11) * ((f + F32(1)) * F32(0.5))
    ok = t >= F32(1)
    return np.where(ok, np.where(t >= F32(10), 10, np.floor(np.where(ok, t, F32(1)))), 0).astype(np.int64)


def bin_theta(x, y, bounds=None):
    """The contract's angle bin of float32 arrays x, y."""
    x = np.asarray(x, F32); y = np.asarray(y, F32)
    up = y >= F32(0)
    b = np.zeros(x.shape, np.int64)
    for k, (bx, by) in enumerate(bounds or theta_bounds(), 1):
        c = bx * y - by * x
        b += ((up | (c >= 0)) if k <= 5 else (up & (c >= 0))).astype(np.int64)
    return b


def numpy_valid(X, N):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isfinite(X).all(1) & np.isfinite(N).all(1) & ((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2] > 0)


def numpy_pairs(X, N, radius, i, valid):
    """(js, d (3, k) float32, d2 (k,) float32) of the pairs of point i."""
    r2 = F32(radius) * F32(radius)
    d = [X[:, a] - X[i, a] for a in range(3)]
    d2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
    js = np.flatnonzero(valid & (d2 > 0) & (d2 <= r2))
    return js, [c[js] for c in d], d2[js]


def numpy_pair_bins(ni, Nj, d, d2):
    """(accepted mask, alpha bins, phi bins, theta bins) of the pairs of one point: ni (3,), Nj (k, 3), d three (k,) arrays."""
    k = len(d2)
    ni = [np.full(k, ni[a], F32) for a in range(3)]
    nj = [Nj[:, a] for a in range(3)]
    ln = np.sqrt(d2)
    ai, aj = _dot(ni, d), _dot(nj, d)
    swap = ~(np.abs(ai) >= np.abs(aj))
    s = [np.where(swap, nj[a], ni[a]) for a in range(3)]
    t = [np.where(swap, ni[a], nj[a]) for a in range(3)]
    e = [np.where(swap, -d[a], d[a]) for a in range(3)]
    phi = _dot(s, e) / ln
    v = [e[1] * s[2] - e[2] * s[1], e[2] * s[0] - e[0] * s[2], e[0] * s[1] - e[1] * s[0]]
    vn = np.sqrt(_dot(v, v))
    acc = vn > 0
    v = [c / vn for c in v]
    w = [s[1] * v[2] - s[2] * v[1], s[2] * v[0] - s[0] * v[2], s[0] * v[1] - s[1] * v[0]]
    return acc, _bin11(_dot(v, t)), _bin11(phi), bin_theta(_dot(s, t), _dot(w, t))


def numpy_fpfh(X, N, radius, want_spfh=False):
    """The contract in numpy and Python integers: (F, count), with want_spfh also S.  Small clouds only: every point is
    tested for every point."""
    X = np.ascontiguousarray(X, F32); N = np.ascontiguousarray(N, F32)
    n = len(X)
    r2 = F32(radius) * F32(radius)
    valid = numpy_valid(X, N)
    Srows = [[0] * BINS for _ in range(n)]
    counts = [0] * n
    pairs = {}
    with np.errstate(all="ignore"):
        for i in np.flatnonzero(valid):
            js, d, d2 = numpy_pairs(X, N, radius, i, valid)
            pairs[i] = (js, d2)
            acc, ba, bp, bt = numpy_pair_bins(N[i], N[js], d, d2)
            H = [0] * BINS
            for b in list(ba[acc]) + list(11 + bp[acc]) + list(22 + bt[acc]):
                H[int(b)] += 1
            c = int(acc.sum())
            counts[i] = c
            if c:
                Srows[i] = [(h << 15) // c for h in H]
        F = np.zeros((n, BINS), np.uint16)
        for i, (js, d2) in pairs.items():
            A = [0] * BINS
            q = np.minimum(F32(64) * (r2 / d2), F32(65536))
            for j, qq in zip(js, q):
                qi = int(qq)
                assert 64 <= qi <= 65536
                for b in range(BINS):
                    A[b] += qi * Srows[j][b]
            for g in range(3):
                T = sum(A[11 * g:11 * g + 11])
                if T:
                    F[i, 11 * g:11 * g + 11] = [int(math.floor((float(a) / float(T)) * 4096.0)) for a in A[11 * g:11 * g + 11]]
    out = (F, np.array(counts, np.int32))
    return out + (np.array(Srows, np.uint16),) if want_spfh else out


def numpy_match(fa, fb, mutual=True):
    """The matcher's contract with Python integers: (idx, dist).  Small tables only."""
    A = [[int(v) for v in row] for row in np.asarray(fa).reshape(-1, BINS)]
    B = [[int(v) for v in row] for row in np.asarray(fb).reshape(-1, BINS)]

    def best(rows, cols):
        out = []
        for r in rows:
            keys = [(sum((x - y) ** 2 for x, y in zip(r, c)), k) for k, c in enumerate(cols) if any(c)] if any(r) else []
            out.append(min(keys) if keys else None)
        return out
    ba = best(A, B)
    bb = best(B, A) if mutual else None
    idx = np.full(len(A), -1, np.int32); dist = np.full(len(A), -1, np.int32)
    for a, key in enumerate(ba):
        if key is not None and (not mutual or bb[key[1]][1] == a):
            dist[a], idx[a] = key
    return idx, dist


# ---- clouds and normals ------------------------------------------------------------------------------------------------------------

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 4097)
cube_cloud, cube_radius, lattice_cloud, below, scale_cloud = SH.cube_cloud, SH.cube_radius, SH.lattice_cloud, SH.below, SH.scale_cloud
large_cloud = CH.large_cloud
LARGE_RADIUS = 0.010                 # about 13 neighbours on the unit sphere with 524 289 points


def random_normals(n, seed=0):
    """n unit normals (float rounding aside) in seeded random directions: every bin of every group is met."""
    v = np.random.default_rng(9100 + seed).normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def radial_normals(X, centre=None):
    """Unit normals pointing away from the centre (default: the mean): outward on a star-shaped surface."""
    X = np.asarray(X, np.float64)
    v = X - (X.mean(0) if centre is None else np.asarray(centre, np.float64))
    ln = np.linalg.norm(v, axis=1, keepdims=True)
    return np.where(ln > 0, v / np.maximum(ln, 1e-300), [[0, 0, 1.0]]).astype(F32)


def plane_lattice(side=12):
    """side x side points of the plane z = 0.25 at integer x, y, permuted, all with the normal (0, 0, 1)."""
    g = np.arange(side, dtype=F32)
    P = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    P = np.concatenate([P, np.full((len(P), 1), 0.25, F32)], 1).astype(F32)
    P = np.ascontiguousarray(P[np.random.default_rng(3).permutation(len(P))])
    return P, np.tile(np.array([[0, 0, 1]], F32), (len(P), 1))


def ball_cloud(n=300, seed=21, radius=0.4):
    """n points uniform in a ball of the given radius: at r = 2 radius every point pairs with every other."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (radius * rng.uniform(0, 1, (n, 1)) ** (1 / 3))).astype(F32)


def mixed_normals(n, seed=5):
    """Random unit normals with zero, NaN, infinite, huge and tiny ones mixed in; (normals, the rows that are not valid)."""
    N = random_normals(n, seed)
    rng = np.random.default_rng(seed)
    rows = rng.choice(n, 12, replace=False)
    N[rows[0]] = 0; N[rows[1]] = [np.nan, 0, 1]; N[rows[2]] = [0, np.inf, 0]; N[rows[3]] = [0, 0, -np.inf]; N[rows[4]] = [np.nan] * 3
    N[rows[5]] = [1e-30, 0, 0]                                  # its squared length underflows to 0: not valid
    N[rows[6]] = [3e38, 3e38, 0]; N[rows[7]] = [1e20, -1e20, 1e20]      # finite, valid; their products overflow
    N[rows[8]] = [1e-18, 0, 0]                                  # valid, far from unit length
    N[rows[9]] = [-0.0, 0.0, -0.0]
    N[rows[10]] = [2, 0, 0]; N[rows[11]] = [0, -0.5, 0]
    return N, np.sort(rows[[0, 1, 2, 3, 4, 5, 9]])


def random_tables(m, n, seed=0, zero_rows=True):
    """Two descriptor tables of m and n rows: random values up to 4096, a few rows of fb copied from fa (exact matches) and
    duplicated (ties), a few rows of zeros on either side."""
    rng = np.random.default_rng(40000 + 131 * m + n + seed)
    fa = rng.integers(0, 4097, size=(m, BINS)).astype(np.uint16); fb = rng.integers(0, 4097, size=(n, BINS)).astype(np.uint16)
    for _ in range(max(1, min(m, n) // 8)):
        fb[rng.integers(0, n)] = fa[rng.integers(0, m)]
    if n >= 4:
        fb[n - 1] = fb[0]; fb[n // 2] = fb[1]
    if zero_rows:
        if m >= 3:
            fa[rng.integers(0, m)] = 0
        if n >= 3:
            fb[rng.integers(0, n)] = 0
    return fa, fb


# ---- the registration pair ---------------------------------------------------------------------------------------------------------

PAIR = dict(n=3000, noise_sigma=0.001, radius=0.08, normal_radius=0.04, max_distance=0.02)


def outward(X, N):
    """N with every normal facing away from the cloud's mean: the sign Normals.orient's "outward" gives a star-shaped cloud."""
    X = np.asarray(X, np.float64)
    flip = ((X - X.mean(0)) * N).sum(1) < 0
    return np.where(flip[:, None], -N, N).astype(F32)


@functools.lru_cache(maxsize=1)
def pair_clouds():
    """(P, Q, T): datasets.bumpy_pair(3000, noise_sigma=0.001); T maps Q onto P."""
    from super4pcs_amd import datasets as D
    return D.bumpy_pair(PAIR["n"], noise_sigma=PAIR["noise_sigma"])


def pair_normals(shape_cpu):
    """The radius normals of both clouds within 0.04 (tests/shape_cpu, the restatement of s4p_shape.h), oriented outward."""
    P, Q, _ = pair_clouds()
    return tuple(outward(Z, shape_cpu.estimate(Z, PAIR["normal_radius"])[0]) for Z in (P, Q))


def rotation_angle_deg(Ta, Tb):
    R = np.asarray(Ta)[:3, :3].T @ np.asarray(Tb)[:3, :3]
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1) / 2))))
