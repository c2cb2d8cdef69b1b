"""The clouds of the grid-regime tests (tests/test_grid_regimes_host.py on the CPU, tests/test_gpu_grid_regimes.py on the
MI355X): degenerate, far and extreme-scale clouds that drive set_cloud's planner (plan_spacing, fit_grid), the neighbour walk
and the clustering grid of libsuper4pcs_normals.so through the branches a unit cube near the origin never reaches.

A case is a function returning (X float32 (n, 3), radius, eps, min_points), seeded and cached (the arrays are read-only).  Its
`regime` attribute is a predicate over Normals.grid() that states, as inequalities, which branch of the planner the cloud is
meant to reach; the GPU test asserts it, so that a change of the planner cannot quietly turn the case into an ordinary cube.
`ext` is the largest extent of the cloud's bounds, or 1 when that is 0.  REFUSED names the cases set_cloud must refuse: their
planned cell edge is below MIN_CELL = 2^-43 (include/s4p_normals.h, Limits)."""
import functools

import numpy as np

MIN_CELL = 2.0 ** -43
FLT_MIN = float(np.finfo(np.float32).tiny)               # 2^-126
SEPARATION_1D = 1000.0                                   # between the centres of two_clusters_1d ("Grid regimes")

CASES = {}


def case(name, regime=None):
    def wrap(fn):
        @functools.lru_cache(maxsize=None)
        def cached():
            X, radius, eps, min_points = fn()
            X = np.ascontiguousarray(X, np.float32)
            assert X.ndim == 2 and X.shape[1] == 3 and np.isfinite(X).all()
            X.setflags(write=False)
            return X, np.float32(radius), np.float32(eps), int(min_points)
        cached.__name__ = name
        cached.regime = regime
        CASES[name] = cached
        return cached
    return wrap


def ext_of(X):
    e = float((X.max(0).astype(np.float64) - X.min(0).astype(np.float64)).max())
    return e if e > 0 else 1.0


def _cube(n, seed):
    return np.random.default_rng(seed).uniform(0, 1, size=(n, 3))


def _ones(g):
    return sum(int(d == 1) for d in g["dims"])


# ---- degenerate shapes -------------------------------------------------------------------------------------------------------

@case("identical", lambda g: g["spacing"] == 0 and g["dims"] == [1, 1, 1] and g["max_per_cell"] == 257 and g["cell"] == 1.0)
def _identical():
    return np.tile(np.array([[0.3, -2.0, 5.0]], np.float32), (257, 1)), 1.0, 0.1, 4


def _line(axis, seed, fixed):
    X = np.empty((257, 3))
    X[:] = fixed
    X[:, axis] = np.random.default_rng(seed).uniform(0, 1, 257)
    return X, 0.02, 0.06, 12


def _line_regime(axis):
    return lambda g: _ones(g) == 2 and g["dims"][axis] >= 8 and 0 < g["spacing"] <= g["cell"] and g["max_per_cell"] < 64


for _a, _name in enumerate(("line_x", "line_y", "line_z")):
    case(_name, _line_regime(_a))(functools.partial(_line, _a, 20 + _a, (0.7, -1.3, 2.5)))


def _plane(axis, seed):
    X = np.random.default_rng(seed).uniform(0, 1, size=(600, 3))
    X[:, axis] = (0.75, -1.5, 3.0)[axis]
    return X, 0.05, 0.11, 24


def _plane_regime(axis):
    return lambda g: g["dims"][axis] == 1 and _ones(g) == 1 and min(d for a, d in enumerate(g["dims"]) if a != axis) >= 8


for _a, _name in enumerate(("plane_x", "plane_y", "plane_z")):
    case(_name, _plane_regime(_a))(functools.partial(_plane, _a, 30 + _a))


@case("diagonal", lambda g: min(g["dims"]) >= 8 and g["nonempty"] * 50 <= g["cells"] and g["nonempty"] <= 3 * max(g["dims"]))
def _diagonal():
    t = np.random.default_rng(40).uniform(0, 1, 257)
    return np.column_stack([t, t, t]), 0.03, 0.1, 12


@case("slab", lambda g: g["dims"][0] >= 8 and g["dims"][1] == 1 and g["dims"][2] == 1)
def _slab():
    return _cube(400, 41) * np.array([1.0, 1e-6, 1e-12]), 0.012, 0.04, 12


# ---- far apart ---------------------------------------------------------------------------------------------------------------

def _two_clusters(n_each, seed, centre):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5e-3, 0.5e-3, size=(n_each, 3))
    b = rng.uniform(-0.5e-3, 0.5e-3, size=(n_each, 3)) + np.asarray(centre, np.float64)
    return np.concatenate([a, b])[rng.permutation(2 * n_each)]


# the cell is the 2^-20 floor of the extent, enlarged once (2^-20 x 1.25 of 1000 gives 838 861 cells): above the spacing, and
# at least 2^19 cells along x, so that an unbounded k = 32 list walks half a million rings or more
@case("two_clusters_1d", lambda g: g["dims"][0] >= 2 ** 19 and g["dims"][1] == 1 and g["dims"][2] == 1 and g["nonempty"] <= 4
      and g["spacing"] < g["cell"])
def _two_clusters_1d():
    return _two_clusters(20, 50, (SEPARATION_1D, 0, 0)), 0.01, 1.7e-3, 5


# the cell cap max(2^20, 4 n) enlarges the cell some thousandfold over the spacing: each cluster sits in one cell
@case("two_clusters_2d", lambda g: g["cell"] >= 1000 * g["spacing"] > 0 and g["max_per_cell"] == 200 and g["nonempty"] == 2
      and g["dims"][2] == 1 and g["cells"] <= 2 ** 20)
def _two_clusters_2d():
    return _two_clusters(200, 51, (1000.0, 1000.0, 0)), 3e-4, 6.4e-4, 12


@case("far_outlier", lambda g: g["max_per_cell"] >= 500 and g["nonempty"] == 2 and g["cell"] > 1.0)
def _far_outlier():
    return np.concatenate([_cube(500, 52), [[1e6, -1e6, 1e6]]]), 0.12, 0.25, 12


def _cube_regime(g):
    """The ordinary grid of a 600-point cube, wherever it lies."""
    return min(g["dims"]) >= 8 and g["max_per_cell"] <= 32 and g["cell"] == g["spacing"]


@case("offset_1e6", lambda g: min(g["dims"]) >= 8 and g["cell"] == g["spacing"])
def _offset_1e6():
    return _cube(600, 53) + 1e6, 0.12, 0.2, 8


@case("offset_neg3e4", _cube_regime)
def _offset_neg3e4():
    return _cube(600, 54) - 3e4, 0.12, 0.2, 8


@case("straddle", _cube_regime)
def _straddle():
    return _cube(600, 55) - np.array([0.5, 0.3, 0.7]), 0.12, 0.2, 8


# ---- the spacing estimate ----------------------------------------------------------------------------------------------------

# bin 0 of the spacing histogram takes every d2 == 0: the estimate collapses, the cell comes from the floor and the cap
@case("dup20", lambda g: 0 < g["spacing"] < 1e-6 and g["cell"] > 1000 * g["spacing"] and 20 <= g["max_per_cell"] <= 60
      and min(g["dims"]) >= 32 and g["cells"] <= 2 ** 20)
def _dup20():
    rng = np.random.default_rng(56)
    X = np.repeat(rng.uniform(0, 1, size=(200, 3)), 20, axis=0)
    return X[rng.permutation(len(X))], 0.1, 1e-9, 20


def _plan_k_regime(g):
    """Fewer than kPlanK = 16 points within reach of the histogram: the L / 32 fallback, a grid of mostly empty cells."""
    return g["spacing"] > 0 and g["cell"] == g["spacing"] and g["cells"] >= 50 * g["nonempty"] and min(g["dims"]) >= 4


for _n in (15, 16, 17):
    case("plan_k_edge_%d" % _n, _plan_k_regime)(functools.partial(lambda n: (_cube(n, 60 + n), 0.3, 0.5, 3), _n))


# ---- scale -------------------------------------------------------------------------------------------------------------------

def _scaled(factor, eps_factor=0.2):
    """The 400-point cube times the factor (float32 product).  An eps whose float square would overflow is capped at 1e19:
    then every point is alone within it."""
    with np.errstate(over="ignore"):
        X = (_cube(400, 70).astype(np.float32) * np.float32(factor)).astype(np.float32)
        eps = min(eps_factor * factor, 1e19)
        return X, np.float32(0.12 * factor), eps, 8


def _scale_regime(g):
    return min(g["dims"]) >= 8 and g["max_per_cell"] <= 32 and g["cell"] >= MIN_CELL


for _name, _f in (("scale_1e-9", 1e-9), ("scale_1e15", 1e15), ("scale_1e18", 1e18), ("scale_3e19", 3e19), ("scale_3e38", 3e38)):
    case(_name, _scale_regime)(functools.partial(_scaled, _f))

# 2^-38: the smallest power of two at which the cube's cell, about 0.054 of the scale, is still accepted
case("scale_limit", lambda g: MIN_CELL <= g["cell"] < 2 * MIN_CELL and min(g["dims"]) >= 8)(functools.partial(_scaled, 2.0 ** -38))

# the cell of the cube at these scales is below MIN_CELL: set_cloud refuses them, so there is no grid to state a regime of.
# At 1e-15 every neighbour's d2 is still a normal float; at 1e-22 they are subnormal or 0
case("scale_1e-15", None)(functools.partial(_scaled, 1e-15))
case("scale_below", None)(functools.partial(_scaled, 1e-22))
REFUSED = ("scale_1e-15", "scale_below")
ACCEPTED = tuple(n for n in CASES if n not in REFUSED)
TWO_CLUSTERS = ("two_clusters_1d", "two_clusters_2d")
PLANES = {"plane_x": 0, "plane_y": 1, "plane_z": 2}
OVERFLOW = ("scale_3e19", "scale_3e38")                  # d2 is +inf for most pairs
ONE_CONTEXT_ORDER = ("dup20", "identical", "two_clusters_1d", "plan_k_edge_16", "far_outlier", "line_z")


def viewpoint(X):
    """A viewpoint at the cloud's scale and place, outside its box in z and finite in float at every scale."""
    lo = X.min(0).astype(np.float64)
    with np.errstate(over="ignore"):
        v = (lo + ext_of(X) * np.array([0.3, -0.2, 1.1])).astype(np.float32)
    assert np.isfinite(v).all()
    return tuple(float(c) for c in v)


def queries(X, seed=9):
    """(Q float32 (m, 3), own): 8 cloud points (own = their indices), the centre and the 8 corners of the bounding box, points
    outside each of the 6 faces at 0.5, 10 and 1000 ext (at most 3.3e38 away from 0, so that every one is finite in float), and
    one non-finite query, last: 36 in all."""
    rng = np.random.default_rng(seed)
    own = rng.integers(0, len(X), 8)
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    ext = ext_of(X)
    c = 0.5 * lo + 0.5 * hi
    rows = [c] + [np.where([(b >> a) & 1 for a in range(3)], hi, lo) for b in range(8)]
    for a in range(3):
        for f in (0.5, 10.0, 1000.0):
            for side in (-1, 1):
                q = c + 0.1 * (hi - lo) * rng.uniform(-1, 1, 3)
                q[a] = (lo[a] - f * ext) if side < 0 else (hi[a] + f * ext)
                rows.append(np.clip(q, -3.3e38, 3.3e38))
    with np.errstate(over="ignore"):
        Q = np.concatenate([X[own], np.array(rows).astype(np.float32), np.array([[np.nan, 0, np.inf]], np.float32)]).astype(np.float32)
    assert np.isfinite(Q[:-1]).all()
    return np.ascontiguousarray(Q), own


# ---- the references, computed once ----------------------------------------------------------------------------------------------

KS = (1, 8, 32)


@functools.lru_cache(maxsize=None)
def reference33(name, bounded):
    """The numpy brute force's 33 nearest of every point of the case (itself included), without or with the case's radius:
    every k <= 32 list, with or without the own index, is a prefix of it (tests/knn_helpers.py lists)."""
    from tests import normals_helpers as NH
    X, radius, _, _ = CASES[name]()
    with np.errstate(over="ignore", invalid="ignore"):
        idx, _ = NH.numpy_knn(X, 33, radius if bounded else None)
    idx.setflags(write=False)
    return idx


def prefix_fn(idx33):
    """A neighbour-set function for knn_helpers.lists that cuts the lists out of the 33 nearest."""
    return lambda X_, k_, r_, queries: (idx33[:, :k_].copy(), (idx33[:, :k_] >= 0).sum(1).astype(np.int32))


def reference_lists(name, k, bounded, exclude_self):
    """(idx, d2, cnt) of the contract for the case's own points."""
    from tests import knn_helpers as KH
    X, radius, _, _ = CASES[name]()
    with np.errstate(over="ignore", invalid="ignore"):
        return KH.lists(prefix_fn(reference33(name, bounded)), X, k, radius if bounded else None, None, exclude_self)


def numpy_density(X, eps):
    """The points with d2 <= fl(eps * eps) around every point, itself included: a count over the float32 distance matrix."""
    out = np.empty(len(X), np.int32)
    with np.errstate(over="ignore"):
        r2 = np.float32(eps) * np.float32(eps)
        for lo in range(0, len(X), 500):
            Q = X[lo:lo + 500]
            dx = X[None, :, 0] - Q[:, None, 0]; dy = X[None, :, 1] - Q[:, None, 1]; dz = X[None, :, 2] - Q[:, None, 2]
            out[lo:lo + 500] = ((dx * dx + (dy * dy + dz * dz)) <= r2).sum(1)
    return out
