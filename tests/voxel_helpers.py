"""Test-side restatement of the voxel-grid downsampling contract (include/s4p_voxel.h): tests/voxel_cpu/voxel_cpu.cpp through
ctypes (a std::map of member lists, explicit loops for the two-level sum), a plain Python dictionary implementation of the
same contract for the tiny shapes, and the clouds the host and GPU tests share.  No numpy reduction is on a reference
path: numpy's pairwise sum has another order."""
import ctypes as C
import math

import numpy as np

from tests import apps
from tests import normals_suite as S
from tests.normals_helpers import bits

MAX_EXTENT = 1 << 21
BLOCK = 64


class ExtentError(ValueError):
    pass


class CPU:
    def __init__(self, L):
        self.L = L

    def downsample(self, X, voxel, attrs=None):
        """(xyz (m, 3) float32, attrs (m, nattr) float32 or None, counts (m,) int32, voxel_of (n,) int32)."""
        p = S.cols(X)
        n = p[0].shape[0]
        A = None if attrs is None else np.ascontiguousarray(np.asarray(attrs, np.float32).reshape(n, -1))
        na = 0 if A is None else A.shape[1]
        xyz = np.empty((n, 3), np.float32); out_a = np.empty((n, max(na, 1)), np.float32)
        cnt = np.empty(n, np.int32); vof = np.empty(n, np.int32)
        m = self.L.voxel_cpu_downsample(*S.xyzn(p), float(voxel), S.ptr(A), na, xyz.ctypes.data, out_a.ctypes.data, cnt.ctypes.data, vof.ctypes.data)
        if m < 0:
            raise ExtentError("an axis spans more than 2^21 voxels")
        return xyz[:m].copy(), (None if A is None else out_a[:m, :na].copy()), cnt[:m].copy(), vof


def build_cpu(outdir):
    L = S.build_restatement("voxel_cpu/voxel_cpu.cpp", outdir, "libvoxel_cpu", openmp=False)
    vp = C.c_void_p
    L.voxel_cpu_downsample.restype = C.c_int64
    L.voxel_cpu_downsample.argtypes = [vp, vp, vp, C.c_int64, C.c_float, vp, C.c_int32, vp, vp, vp, vp]
    return CPU(L)


def two_level(values):
    """The contract's sum of a list of Python floats (doubles): blocks of 64 in order, then the blocks' sums in order."""
    S = None
    for b in range(0, len(values), BLOCK):
        s = values[b]
        for t in values[b + 1:b + BLOCK]:
            s += t
        S = s if S is None else S + s
    return S


def sequential(values):
    s = values[0]
    for t in values[1:]:
        s += t
    return s


def dict_downsample(X, voxel, attrs=None):
    """The contract with a Python dictionary and Python floats; same returns as CPU.downsample."""
    X = np.asarray(X, np.float32)
    n = len(X)
    A = None if attrs is None else np.asarray(attrs, np.float32).reshape(n, -1)
    v = float(np.float32(voxel))
    cells = {}
    for i in range(n):
        p = [float(t) for t in X[i]]
        if not all(math.isfinite(t) for t in p):
            continue
        key = (math.floor(p[2] / v), math.floor(p[1] / v), math.floor(p[0] / v))
        cells.setdefault(key, []).append(i)
    vof = np.full(n, -1, np.int32)
    xyz, out_a, cnt = [], [], []
    for r, key in enumerate(sorted(cells)):
        mem = cells[key]
        c = float(len(mem))
        xyz.append([np.float32(two_level([float(X[i, a]) for i in mem]) / c) for a in range(3)])
        if A is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                out_a.append([np.float32(two_level([float(A[i, a]) for i in mem]) / c) for a in range(A.shape[1])])
        cnt.append(len(mem))
        vof[mem] = r
    m = len(cnt)
    return (np.array(xyz, np.float32).reshape(m, 3), None if A is None else np.array(out_a, np.float32).reshape(m, A.shape[1]),
            np.array(cnt, np.int32), vof)


CRAFTED_SEED = 20                     # the seed of crafted_values: checked in tests/test_voxel_host.py
CRAFTED_COUNT = 200


def crafted_values(count=CRAFTED_COUNT, seed=CRAFTED_SEED):
    """float32 values of mixed magnitude that cancel: 2/5 of them large (1e12 .. 1e15), each with its negative, the rest in
    (0, 1), shuffled.  The exact sum is the small values' sum; a computed sum depends on the order of the additions."""
    rng = np.random.default_rng(seed)
    nbig = (2 * count // 5) // 2
    big = (10.0 ** rng.uniform(12, 15, nbig)).astype(np.float32)
    vals = np.concatenate([big, -big, rng.uniform(0, 1, count - 2 * nbig).astype(np.float32)])
    return vals[rng.permutation(count)]


def attrs_for(n, nattr, seed):
    """n x nattr float32 attributes; channel 0 holds the cancelling values, so that the order of a voxel's sum shows."""
    if nattr == 0:
        return None
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, nattr)).astype(np.float32)
    A[:, 0] = crafted_values(n, seed) if n >= 5 else A[:, 0]
    return A


def one_voxel(c, nattr=3):
    """c points inside the voxel [0, 1)^3 at voxel size 1, between 7 points in voxels before it and 5 after it in the output
    order, the whole shuffled.  Channel 0 of the voxel's own members holds crafted_values(c): the order of its sum shows."""
    rng = np.random.default_rng(100 + c)
    inside = rng.uniform(0.05, 0.95, size=(c, 3))
    before = rng.uniform(0.05, 0.95, size=(7, 3)) + np.array([0, 0, -2.0])
    after = rng.uniform(0.05, 0.95, size=(5, 3)) + np.array([3.0, 1.0, 0])
    A = rng.normal(size=(c + 12, nattr)).astype(np.float32)
    if c >= 5:
        A[:c, 0] = crafted_values(c, 100 + c)                # the cancelling values are the voxel's own members
    perm = rng.permutation(c + 12)
    return np.concatenate([inside, before, after])[perm].astype(np.float32), 1.0, A[perm]


def _random(n, nattr, voxel=0.5, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(2000 + n)
    X = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    return X, voxel, attrs_for(n, nattr, 2000 + n)


def _lattice():
    """Points exactly on voxel faces (multiples of the voxel size 0.25), negative coordinates and -0.0 included, each
    twice, and points just below the faces: floor, not truncation."""
    g = np.arange(-4, 5, dtype=np.float32) * np.float32(0.25)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    below = np.nextafter(X[::3], np.float32(-np.inf))
    X = np.concatenate([X, X[::2], below, np.array([[-0.0, -0.0, -0.0], [-0.0, 0.0, -0.0]], np.float32)]).astype(np.float32)
    X = X[np.random.default_rng(4).permutation(len(X))]
    return X, 0.25, attrs_for(len(X), 1, 4)


def _duplicates():
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    X[200:] = X[rng.integers(0, 200, 100)]
    return X, 0.3, attrs_for(300, 3, 5)


def _nonfinite():
    rng = np.random.default_rng(6)
    X = rng.uniform(-1, 1, size=(257, 3)).astype(np.float32)
    X[::7, 0] = np.nan; X[3::11, 1] = np.inf; X[5::13, 2] = -np.inf; X[256] = np.nan
    A = attrs_for(257, 3, 6)
    A[10:20, 1] = np.nan                      # a NaN attribute is taken as it is: a NaN mean
    return X, 0.4, A


def _all_nonfinite():
    X = np.full((70, 3), np.nan, np.float32)
    X[::2, 1] = np.inf; X[1::2] = [0.0, -np.inf, 1.0]
    return X, 0.5, attrs_for(70, 1, 7)


def _wide_keys():
    """A few hundred points over nearly 2^21 voxels per axis: the packed key uses all of its 63 bits."""
    rng = np.random.default_rng(8)
    X = rng.uniform(-1000, 1000, size=(400, 3)).astype(np.float32)
    X[300:] = X[:100] + np.float32(0.0002)
    return X, 0.001, attrs_for(400, 1, 8)


CASES = {
    "n1": lambda: _random(1, 0), "n2": lambda: _random(2, 1), "n63": lambda: _random(63, 3), "n64": lambda: _random(64, 8),
    "n65": lambda: _random(65, 0), "n257": lambda: _random(257, 3),
    "one1": lambda: one_voxel(1), "one63": lambda: one_voxel(63), "one64": lambda: one_voxel(64), "one65": lambda: one_voxel(65),
    "one128": lambda: one_voxel(128), "one129": lambda: one_voxel(129), "one4097": lambda: one_voxel(4097, 8),
    "lattice": _lattice, "around1e4": lambda: _random(300, 1, voxel=0.7, lo=9990.0, hi=10010.0), "duplicates": _duplicates,
    "nonfinite": _nonfinite, "all_nonfinite": _all_nonfinite, "tiny_voxel": lambda: _random(257, 1, voxel=1e-6, lo=0.0, hi=1.0),
    "attr0": lambda: _random(200, 0, voxel=0.4), "attr1": lambda: _random(201, 1, voxel=0.4), "attr3": lambda: _random(202, 3, voxel=0.4),
    "attr8": lambda: _random(203, 8, voxel=0.4), "wide_keys": _wide_keys,
}
TINY = [k for k in CASES if k != "one4097"]                 # what the Python dictionary implementation is run on


def assert_same(got, want, what):
    """Bit equality of (xyz, attrs, counts, voxel_of) and of m."""
    gx, ga, gc, gv = [None if t is None else S.to_host(t) for t in got]
    wx, wa, wc, wv = want
    assert gx.shape == wx.shape, (what, "m", gx.shape, wx.shape)
    assert np.array_equal(gc, wc), (what, "counts")
    assert np.array_equal(gv, wv), (what, "voxel_of")
    bad = np.flatnonzero((bits(gx) != bits(wx)).any(1))
    assert len(bad) == 0, (what, "xyz", bad[:5], gx[bad[:3]], wx[bad[:3]], wc[bad[:3]])
    assert (ga is None) == (wa is None), (what, "attrs")
    if wa is not None:
        bad = np.flatnonzero((bits(ga) != bits(wa)).any(1))
        assert len(bad) == 0, (what, "attrs", bad[:5], ga[bad[:3]], wa[bad[:3]], wc[bad[:3]])


write_obj = apps.write_obj


write_table = apps.write_xyz
