"""ctypes binding of include/s4p_icp.h, include/s4p_icp_plane.h, include/s4p_icp_robust.h, include/s4p_icp_gicp.h,
include/s4p_icp_symm.h, include/s4p_icp_color.h, include/s4p_icp_reject.h, include/s4p_icp_batch.h and include/s4p_icp_info.h
(libsuper4pcs_icp.so):
point-to-point, point-to-plane, generalized (plane-to-plane), symmetric and coloured ICP refinement on the full-resolution clouds, with optional robust
losses for the first two, optional correspondence rejection (reciprocal pairs, normal angle) for all of them, and batched
multi-start refinement (many start poses in one pass, ranked on the full clouds) for the first two.

    from super4pcs_amd import icp
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta)     # T maps Q onto P (caller frame, float64 4x4)
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta, metric="plane")   # target normals estimated on the device
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta, loss="trimmed", trim_fraction=0.6)   # trimmed ICP
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta, metric="gicp")    # normals of both clouds (given or estimated)
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta, metric="symmetric")   # the same normals, a wider basin than "plane"
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta, metric="color", target_intensity=rgbP, source_intensity=rgbQ)
    T, res = icp.refine(P, Q, T0, max_distance=4 * delta, reciprocal=True, normal_angle=60)   # pair rejection, any metric / loss
    T, res, i = icp.refine_best(P, Q, T0s, max_distance=4 * delta)          # up to 64 starts side by side; the best by n_corr, rmse
    info, n, rmse = icp.information(P, Q, T, max_distance=4 * delta)        # the 6x6 weight of this pair in a pose graph

Clouds are (N, 3) float32 numpy arrays, or contiguous (N, 3) float32 torch tensors on the context's GPU (they enter
through the *_device entry points, device to device).  There is no CPU fallback: without a device, ICP() raises
ICPError with code -2.
"""
import contextlib
import ctypes as C
import os

import numpy as np

from . import _binding as _B
from . import posegraph as _PG          # its table and structures; posegraph states them before it imports this module
from ._binding import TWIN

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsuper4pcs_icp.so")

NSUMS = 17
PLANE_NSUMS = 31
HISTORY = 64
MAX_ITERATIONS, CONVERGED, TOO_FEW, DEGENERATE = 0, 1, 2, 3
STATUS_NAMES = {MAX_ITERATIONS: "max iterations", CONVERGED: "converged", TOO_FEW: "too few correspondences",
                DEGENERATE: "degenerate plane system"}
ERR_DEGENERATE = -8
ERR_NAMES = {0: "OK", -1: "BAD_ARG", -2: "NO_DEVICE", -3: "HIP", -4: "OOM", -7: "STATE", ERR_DEGENERATE: "DEGENERATE"}
METRICS = ("point", "plane")
REFINE_METRICS = METRICS + ("gicp", "symmetric", "color")   # include/s4p_icp_gicp.h, _symm.h, _color.h: no robust losses
NORMAL_PAIR_METRICS = ("gicp", "symmetric")      # the metrics on the normals of both clouds
GICP_NSUMS = PLANE_NSUMS
SYMM_NSUMS = PLANE_NSUMS
GICP_EPSILON = 1e-3
COLOR_NSUMS = PLANE_NSUMS
COLOR_LAMBDA = 0.968            # S4P_ICP_COLOR_LAMBDA: the weight of the geometric term
COLOR_MIN_NEIGHBOURS = 4        # the smallest min_neighbours of estimate_color_gradients
MIN_NEIGHBOURS = 6              # estimate_normals' default
LOSSES = {"trimmed": 1, "huber": 2, "tukey": 3}             # S4P_ICP_LOSS_*
LOSS_C = {"huber": 1.345, "tukey": 4.685}                   # default tuning constants
ROBUST_NINFO = 8

BATCH_MAX = 64                                             # S4P_ICP_BATCH_MAX
INFO_NSUMS = 11                                            # S4P_ICP_INFO_NSUMS
NORMALS_OFF, NORMALS_UNORIENTED, NORMALS_ORIENTED = 0, 1, 2         # S4P_ICP_REJECT_NORMALS_*
WHY_KEPT, WHY_UNMATCHED, WHY_NORMALS, WHY_RECIPROCITY = 0, 1, 2, 3  # S4P_ICP_WHY_*


class ICPError(RuntimeError):
    REBUILD = "build.build_icp()"

    def __init__(self, code, msg):
        super().__init__("s4p_icp error %s (%d): %s" % (ERR_NAMES.get(code, "?"), code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("min_correspondences", C.c_int32), ("rel_tol", C.c_double),
                ("order_source", C.c_int32), ("reserved", C.c_int32)]


class BatchParams(C.Structure):
    _fields_ = [("icp", Params), ("metric", C.c_int32), ("reserved", C.c_int32)]


class Robust(C.Structure):
    _fields_ = [("loss", C.c_int32), ("reserved0", C.c_int32), ("trim_fraction", C.c_double), ("scale", C.c_double),
                ("c", C.c_double), ("reserved", C.c_double * 4)]


class Reject(C.Structure):
    _fields_ = [("reciprocal", C.c_int32), ("normal_mode", C.c_int32), ("normal_cos", C.c_double), ("reserved", C.c_double * 4)]


class Result(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("n_corr", C.c_int64), ("rmse", C.c_double),
                ("fitness", C.c_double), ("history_len", C.c_int32), ("reserved", C.c_int32),
                ("history_rmse", C.c_double * HISTORY), ("history_n", C.c_int64 * HISTORY)]

    def as_dict(self):
        k = self.history_len
        return {"iterations": self.iterations, "status": STATUS_NAMES[self.status], "n_corr": self.n_corr, "rmse": self.rmse,
                "fitness": self.fitness, "history_rmse": list(self.history_rmse[:k]), "history_n": list(self.history_n[:k])}


_VP, _FP, _DP, _IP, _LP = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
_PARAMS, _RESULT = C.POINTER(Params), C.POINTER(Result)
SIGNATURES = {                                             # include/s4p_icp.h
    "s4p_icp_default_params": (None, [_PARAMS]),
    "s4p_icp_create": [C.c_int32, C.POINTER(_VP)],
    "s4p_icp_destroy": (None, [_VP]),
    "s4p_icp_last_error": (C.c_char_p, [_VP]),
    "s4p_icp_set_target" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64, C.c_float],
    "s4p_icp_set_source" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64],
    "s4p_icp_frame": [_VP, _FP],
    "s4p_icp_correspondences": [_VP, _FP, _IP, _FP],
    "s4p_icp_sums": [_VP, _FP, _DP],
    "s4p_icp_solve": [_DP, _DP],
    "s4p_icp_refine": [_VP, _PARAMS, _DP, _RESULT],
    "s4p_icp_apply": [_VP, _DP, _FP, _FP, _FP, C.c_int64],
}
PLANE_SIGNATURES = {                                       # include/s4p_icp_plane.h
    "s4p_icp_set_target_normals" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64],
    "s4p_icp_estimate_normals": [_VP, C.c_float, C.c_int32],
    "s4p_icp_target_normals": [_VP, _FP, _FP, _FP],
    "s4p_icp_plane_sums": [_VP, _FP, _DP],
    "s4p_icp_solve_plane": [_DP, _DP],
    "s4p_icp_refine_plane": [_VP, _PARAMS, _DP, _RESULT],
}
ROBUST_SIGNATURES = {                                      # include/s4p_icp_robust.h
    "s4p_icp_robust_defaults": (None, [C.POINTER(Robust), C.c_int32]),
    "s4p_icp_robust_sums": [_VP, _FP, C.c_int32, C.POINTER(Robust), _DP, _DP],
    "s4p_icp_refine_robust": [_VP, _PARAMS, C.c_int32, C.POINTER(Robust), _DP, _RESULT, _DP],
}
GICP_SIGNATURES = {                                        # include/s4p_icp_gicp.h
    "s4p_icp_set_source_normals" + TWIN: [_VP, _VP, _VP, _VP, C.c_int64],
    "s4p_icp_source_normals": [_VP, _FP, _FP, _FP],
    "s4p_icp_gicp_sums": [_VP, _FP, C.c_double, _DP],
    "s4p_icp_refine_gicp": [_VP, _PARAMS, C.c_double, _DP, _RESULT],
}
SYMM_SIGNATURES = {                                        # include/s4p_icp_symm.h
    "s4p_icp_symm_sums": [_VP, _FP, _DP],
    "s4p_icp_solve_symmetric": [_DP, _DP],
    "s4p_icp_refine_symm": [_VP, _PARAMS, _DP, _RESULT],
}
COLOR_SIGNATURES = {                                       # include/s4p_icp_color.h
    "s4p_icp_set_target_intensity" + TWIN: [_VP, _VP, C.c_int64],
    "s4p_icp_set_source_intensity" + TWIN: [_VP, _VP, C.c_int64],
    "s4p_icp_estimate_color_gradients": [_VP, C.c_float, C.c_int32],
    "s4p_icp_target_color_gradients": [_VP, _FP, _FP, _FP],
    "s4p_icp_color_sums": [_VP, _FP, C.c_double, _DP],
    "s4p_icp_refine_color": [_VP, _PARAMS, C.c_double, _DP, _RESULT],
}
REJECT_SIGNATURES = {                                      # include/s4p_icp_reject.h
    "s4p_icp_reject_defaults": (None, [C.POINTER(Reject)]),
    "s4p_icp_set_rejection": [_VP, C.POINTER(Reject)],
    "s4p_icp_rejection": [_VP, _FP, _IP, _FP, _IP],
    "s4p_icp_rejection_counts": [_VP, _LP],
}
BATCH_SIGNATURES = {                                       # include/s4p_icp_batch.h
    "s4p_icp_sums_batch": [_VP, C.c_int32, C.c_int32, _FP, _DP],
    "s4p_icp_refine_batch": [_VP, C.POINTER(BatchParams), C.c_int32, _DP, _RESULT, _IP],
    "s4p_icp_rank_batch": [_RESULT, C.c_int32, _IP],
}
INFO_SIGNATURES = {                                        # include/s4p_icp_info.h
    "s4p_icp_information_sums": [_VP, _FP, _DP],
    "s4p_icp_information_from_sums": [_DP, _FP, _DP, _LP, _DP],
    "s4p_icp_information": [_VP, _DP, _DP, _LP, _DP],
}
TABLES = (SIGNATURES, PLANE_SIGNATURES, ROBUST_SIGNATURES, GICP_SIGNATURES, SYMM_SIGNATURES, COLOR_SIGNATURES, REJECT_SIGNATURES,
          BATCH_SIGNATURES, INFO_SIGNATURES, _PG.SIGNATURES)           # the last: include/s4p_icp_posegraph.h
(SYMBOLS, PLANE_SYMBOLS, ROBUST_SYMBOLS, GICP_SYMBOLS, SYMM_SYMBOLS, COLOR_SYMBOLS, REJECT_SYMBOLS, BATCH_SYMBOLS, INFO_SYMBOLS,
 POSEGRAPH_SYMBOLS) = (_B.names(t) for t in TABLES)

_LOADED = {}           # library path -> (the library, the tables declared on it): _binding.load


def load_library(path=None):
    """The library at path (default LIB_PATH), opened once per process, with every table declared; a library without one of
    their functions is an error."""
    return _B.load(_LOADED, path or LIB_PATH, TABLES, ICPError, "libsuper4pcs_icp.so")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _host_solve(name, nsums, sums, refused=None):
    """s4p_icp_<name>(sums, dT) on the host: the 4x4 dT, or ICPError with `refused` (default: degenerate system / bad argument)."""
    fn = getattr(load_library(), "s4p_icp_" + name)
    s = np.ascontiguousarray(sums, np.float64).reshape(nsums)
    out = np.empty(16, np.float64)
    rc = fn(_dp(s), _dp(out))
    if rc != 0:
        raise ICPError(rc, refused or name + (": degenerate system" if rc == ERR_DEGENERATE else ": bad argument"))
    return out.reshape(4, 4)


def solve(sums):
    """Horn's closed form on the 17 sums (host only, no device): the 4x4 dT mapping q^ onto p'."""
    return _host_solve("solve", NSUMS, sums, "solve: n < 1")


def solve_plane(sums):
    """The point-to-plane step on the 31 plane sums (host only, no device): dT = [Rodrigues(omega) | t] with A (omega, t) = b.
    Raises ICPError with code ERR_DEGENERATE when n_plane < 6 or A is not safely positive definite."""
    return _host_solve("solve_plane", PLANE_NSUMS, sums)


def solve_symmetric(sums):
    """The symmetric step on the 31 symmetric sums (host only, no device; include/s4p_icp_symm.h): with A (a, t) = b solved
    as solve_plane solves it and Rh the rotation by atan |a| about a, dT = [Rh Rh | Rh (cos(atan |a|) t)].  Raises ICPError
    with code ERR_DEGENERATE where solve_plane does."""
    return _host_solve("solve_symmetric", SYMM_NSUMS, sums)


def robust_params(loss, trim_fraction=None, scale=None, c=None):
    """The s4p_icp_robust of a loss name: "trimmed" needs trim_fraction in (0, 1]; "huber" / "tukey" take scale (> 0 fixed,
    None or <= 0 estimated on the device) and c (None: 1.345 / 4.685).  A parameter the loss does not use is an error."""
    if loss not in LOSSES:
        raise ValueError("loss must be one of %s" % (tuple(LOSSES),))
    r = Robust()
    load_library().s4p_icp_robust_defaults(C.byref(r), LOSSES[loss])
    if loss == "trimmed":
        if scale is not None or c is not None:
            raise ValueError("the trimmed loss takes no scale or c")
        if trim_fraction is None:
            raise ValueError("the trimmed loss needs trim_fraction")
        r.trim_fraction = float(trim_fraction)
    else:
        if trim_fraction is not None:
            raise ValueError("trim_fraction belongs to the trimmed loss")
        if scale is not None:
            r.scale = float(scale)
        if c is not None:
            r.c = float(c)
    return r


def reject_params(reciprocal=False, normal_angle=None, oriented=False):
    """The s4p_icp_reject of (reciprocal, normal_angle in degrees or None, oriented): the cosine is math.cos of the angle in
    double.  The angle must be in [0, 90] for unoriented normals and in [0, 180] for oriented ones."""
    import math
    r = Reject()
    load_library().s4p_icp_reject_defaults(C.byref(r))
    r.reciprocal = int(bool(reciprocal))
    if normal_angle is None:
        if oriented:
            raise ValueError("oriented needs normal_angle")
        return r
    a = float(normal_angle)
    if not (0.0 <= a <= (180.0 if oriented else 90.0)):
        raise ValueError("normal_angle must be in [0, %d] degrees" % (180 if oriented else 90))
    r.normal_mode = NORMALS_ORIENTED if oriented else NORMALS_UNORIENTED
    r.normal_cos = min(1.0, max(-1.0 if oriented else 0.0, math.cos(math.radians(a))))
    return r


def compose(A, B):
    """A @ B for 4x4 float64 in the facade's order (sum over k = 0..3 left to right, no fused multiply-add), so that a
    matrix composed here equals the one RefineICP / the command line composes."""
    A = np.asarray(A, np.float64); B = np.asarray(B, np.float64)
    out = np.empty((4, 4), np.float64)
    for a in range(4):
        for b in range(4):
            v = 0.0
            for k in range(4):
                v += float(A[a, k]) * float(B[k, b])
            out[a, b] = v
    return out


def _batch_metric(metric):
    if metric not in METRICS:
        raise ValueError("a batch refines metric \"point\" or \"plane\" (robust losses, \"gicp\", \"symmetric\" and \"color\" have no batch form)")
    return METRICS.index(metric)


def _batch_transforms(Ts, dtype):
    """(B, 4, 4) contiguous of the given type from B transforms, 1 <= B <= BATCH_MAX."""
    T = np.ascontiguousarray(np.asarray(Ts, dtype))
    if T.ndim == 2 and T.shape == (4, 4):
        T = T.reshape(1, 4, 4)
    if T.ndim != 3 or T.shape[1:] != (4, 4):
        raise ValueError("the transforms of a batch are (B, 4, 4)")
    if not (1 <= T.shape[0] <= BATCH_MAX):
        raise ValueError("a batch holds 1..%d transforms, not %d" % (BATCH_MAX, T.shape[0]))
    return T.copy()


def rank_batch(results):
    """int32 (B,): the order of include/s4p_icp_batch.h over a sequence of Result -- n_corr descending, then rmse ascending,
    then the index; poses without a correspondence last.  Host only, needs no device."""
    L = load_library()
    B = len(results)
    arr = (Result * max(B, 1))(*results)
    order = np.empty(max(B, 1), np.int32)
    rc = L.s4p_icp_rank_batch(arr, B, order.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise ICPError(rc, "rank_batch: 1..%d results" % BATCH_MAX)
    return order


def _check_metric(metric, loss):
    if metric not in REFINE_METRICS:
        raise ValueError("metric must be one of %s" % (REFINE_METRICS,))
    if metric in ("gicp", "symmetric", "color") and loss is not None:
        raise ValueError("metric \"%s\" takes no loss (robust losses cover \"point\" and \"plane\")" % metric)


def rgb_to_intensity(rgb):
    """float32 (n,): ((double r + double g) + double b) / 765 of an (n, 3) rgb array in 0..255 (numpy, or a torch tensor,
    which stays on its device) -- the formula of the facade (include/super4pcs/algorithms/icp.h)."""
    if _B.is_torch(rgb):
        import torch
        if rgb.dim() != 2 or rgb.shape[1] != 3:
            raise ValueError("rgb is (N, 3)")
        d = rgb.to(torch.float64)
        return (((d[:, 0] + d[:, 1]) + d[:, 2]) / 765.0).to(torch.float32)
    d = np.asarray(rgb, np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError("rgb is (N, 3)")
    return (((d[:, 0] + d[:, 1]) + d[:, 2]) / 765.0).astype(np.float32)


def _as_intensity(v):
    """One float per point: an (n, 3) input is rgb and goes through rgb_to_intensity, an (n,) or (n, 1) one is taken as it is."""
    if not _B.is_torch(v):
        v = np.asarray(v)
    nd = v.dim() if _B.is_torch(v) else v.ndim
    if nd == 2 and v.shape[1] == 3:
        return rgb_to_intensity(v)
    if nd == 2 and v.shape[1] == 1:
        return v[:, 0]
    if nd != 1:
        raise ValueError("an intensity is (N,) or (N, 1), a colour (N, 3)")
    return v


class ICP:
    """One s4p_icp context (one GPU)."""

    def __init__(self, device=0, lib=None):
        """lib: the path of another copy or build of the library, bound next to the package's (None)."""
        self.L = load_library(lib)
        self.device = device
        h = C.c_void_p()
        rc = self.L.s4p_icp_create(device, C.byref(h))
        if rc != 0:
            raise ICPError(rc, self.L.s4p_icp_last_error(None).decode())
        self.h = h
        self.n_p = 0
        self.n_q = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.s4p_icp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise ICPError(rc, self.L.s4p_icp_last_error(self.h).decode())

    def _upload(self, name, X, *tail):
        """n of the (n, 3) numpy array or GPU torch tensor X after `name`(h, x, y, z, n, *tail), or its _device twin, on X's
        columns."""
        dev, ptr, n, keep = _B.cols(X)
        self._chk(getattr(self.L, name + "_device" if dev else name)(self.h, *ptr, n, *tail))
        return n

    def set_target(self, P, max_distance):
        self.n_p = self._upload("s4p_icp_set_target", P, float(max_distance))

    def set_source(self, Q):
        self.n_q = self._upload("s4p_icp_set_source", Q)

    def frame(self):
        c = np.empty(3, np.float32)
        self._chk(self.L.s4p_icp_frame(self.h, _fp(c)))
        return c

    @staticmethod
    def _t32(T):
        T = np.ascontiguousarray(np.asarray(T).reshape(4, 4), np.float32).reshape(16)
        return T

    def _read3(self, fn, n):
        """float32 (n, 3): the three columns that fn(h, x, y, z) fills."""
        cols = [np.empty(n, np.float32) for _ in range(3)]
        self._chk(fn(self.h, _fp(cols[0]), _fp(cols[1]), _fp(cols[2])))
        return np.stack(cols, axis=1)

    def _sums(self, fn, T, n, *scalar):
        """float64 (n,): fn(h, float T, [scalar,] out) for a T in the centred frame."""
        T = self._t32(T)
        out = np.empty(n, np.float64)
        self._chk(fn(self.h, _fp(T), *scalar, _dp(out)))
        return out

    def set_target_normals(self, N):
        """One normal per target point (N, 3), in the uploaded order: normalised in double, zero / non-finite -> 0."""
        self._upload("s4p_icp_set_target_normals", N)

    def estimate_normals(self, radius, min_neighbours=MIN_NEIGHBOURS):
        """Target normals on the device from the neighbours within radius (0 < radius <= max_distance)."""
        self._chk(self.L.s4p_icp_estimate_normals(self.h, float(radius), int(min_neighbours)))

    def target_normals(self):
        """float32 (n_P, 3): the current target normals, in the uploaded order."""
        return self._read3(self.L.s4p_icp_target_normals, self.n_p)

    def plane_sums(self, T):
        """The 31 plane sums for a float T in the centred frame (layout in include/s4p_icp_plane.h)."""
        return self._sums(self.L.s4p_icp_plane_sums, T, PLANE_NSUMS)

    def set_source_normals(self, N):
        """One normal per source point (N, 3), in the uploaded order and the frame of the source as uploaded (the library
        rotates them with T): normalised in double, zero / non-finite -> 0.  set_source invalidates them."""
        self._upload("s4p_icp_set_source_normals", N)

    def source_normals(self):
        """float32 (n_Q, 3): the stored source normals, in the uploaded order."""
        return self._read3(self.L.s4p_icp_source_normals, self.n_q)

    def gicp_sums(self, T, epsilon=GICP_EPSILON):
        """The 31 generalized sums for a float T in the centred frame (layout in include/s4p_icp_gicp.h)."""
        return self._sums(self.L.s4p_icp_gicp_sums, T, GICP_NSUMS, float(epsilon))

    def symmetric_sums(self, T):
        """The 31 symmetric sums for a float T in the centred frame (layout in include/s4p_icp_symm.h)."""
        return self._sums(self.L.s4p_icp_symm_sums, T, SYMM_NSUMS)

    def _scalars(self, v):
        """(entry-point suffix, pointer, n, keep-alive) of one float per point: numpy, or a torch tensor on the GPU."""
        if _B.is_torch(v):
            import torch
            if not (v.is_cuda and v.dim() == 1):
                raise ValueError("torch input must be a (N,) tensor on the GPU")
            c = v.to(torch.float32).contiguous()
            _B.sync(v)                                # the copy runs on torch's stream; the library reads on its own
            return "_device", c.data_ptr(), int(c.shape[0]), c
        c = np.ascontiguousarray(v, dtype=np.float32)
        if c.ndim != 1:
            raise ValueError("an intensity is (N,)")
        return "", c.ctypes.data, int(c.shape[0]), c

    def set_target_intensity(self, I):
        """One finite float per target point (N,), in the uploaded order (include/s4p_icp_color.h).  Invalidates the gradients."""
        suf, ptr, n, keep = self._scalars(I)
        self._chk(getattr(self.L, "s4p_icp_set_target_intensity" + suf)(self.h, ptr, n))
        del keep

    def set_source_intensity(self, I):
        """One finite float per source point (N,), in the uploaded order.  set_source invalidates it."""
        suf, ptr, n, keep = self._scalars(I)
        self._chk(getattr(self.L, "s4p_icp_set_source_intensity" + suf)(self.h, ptr, n))
        del keep

    def estimate_color_gradients(self, radius, min_neighbours=MIN_NEIGHBOURS):
        """The intensity gradient of every target point in its tangent plane, on the device, from the neighbours within
        radius (0 < radius <= max_distance, min_neighbours >= 4).  Needs target normals and target intensity."""
        self._chk(self.L.s4p_icp_estimate_color_gradients(self.h, float(radius), int(min_neighbours)))

    def target_color_gradients(self):
        """float32 (n_P, 3): the current gradients, in the uploaded order."""
        return self._read3(self.L.s4p_icp_target_color_gradients, self.n_p)

    def color_sums(self, T, color_lambda=COLOR_LAMBDA):
        """The 31 joint sums for a float T in the centred frame (layout in include/s4p_icp_color.h)."""
        return self._sums(self.L.s4p_icp_color_sums, T, COLOR_NSUMS, float(color_lambda))

    def set_rejection(self, reciprocal=False, normal_angle=None, oriented=False, normal_cos=None):
        """The context's pair rejection (include/s4p_icp_reject.h): reciprocal keeps a pair only if the source point is the
        nearest one of its target point too; normal_angle (degrees) keeps a pair only if the target normal and the rotated
        source normal are at most that far apart (oriented=False: up to sign).  normal_cos gives the cosine itself instead
        of the angle.  Everything False / None turns it off.  Every sums call and every refine honours it."""
        if normal_cos is not None:
            if normal_angle is not None:
                raise ValueError("normal_angle or normal_cos, not both")
            r = reject_params(reciprocal)
            r.normal_mode = NORMALS_ORIENTED if oriented else NORMALS_UNORIENTED
            r.normal_cos = float(normal_cos)
        else:
            r = reject_params(reciprocal, normal_angle, oriented)
        self._chk(self.L.s4p_icp_set_rejection(self.h, C.byref(r)))

    def rejection(self, T):
        """(idx int32[n_Q], d2 float32[n_Q], why int32[n_Q]) for a float T in the centred frame under the context's
        rejection: why 0 kept, 1 unmatched, 2 rejected by normals, 3 by reciprocity; idx -1 and d2 0 unless kept."""
        T = self._t32(T)
        idx = np.empty(self.n_q, np.int32); d2 = np.empty(self.n_q, np.float32); why = np.empty(self.n_q, np.int32)
        ip = C.POINTER(C.c_int32)
        self._chk(self.L.s4p_icp_rejection(self.h, _fp(T), idx.ctypes.data_as(ip), _fp(d2), why.ctypes.data_as(ip)))
        return idx, d2, why

    def rejection_counts(self):
        """int64[4] of the last pass under rejection: matched one-way, rejected by normals, by reciprocity, kept."""
        out = np.zeros(4, np.int64)
        self._chk(self.L.s4p_icp_rejection_counts(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def correspondences(self, T):
        """(idx int32[n_Q], d2 float32[n_Q]) for a float T in the centred frame; idx -1 where nothing is within d."""
        T = self._t32(T)
        idx = np.empty(self.n_q, np.int32); d2 = np.empty(self.n_q, np.float32)
        self._chk(self.L.s4p_icp_correspondences(self.h, _fp(T), idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(d2)))
        return idx, d2

    def sums(self, T):
        """The 17 double sums for a float T in the centred frame: n, sum q^, sum p', sum q^ p'^T (row-major), sum d2."""
        return self._sums(self.L.s4p_icp_sums, T, NSUMS)

    def robust_sums(self, T, metric, loss, trim_fraction=None, scale=None, c=None):
        """(sums, info) for a float T in the centred frame: the weighted 17 (point) or 31 (plane) sums and the 8 info
        doubles of include/s4p_icp_robust.h (M, k, threshold key bits, s, count with w > 0, sum w, 0, 0)."""
        if metric not in METRICS:
            raise ValueError("metric must be one of %s" % (METRICS,))
        r = robust_params(loss, trim_fraction, scale, c)
        T = self._t32(T)
        out = np.empty(PLANE_NSUMS if metric == "plane" else NSUMS, np.float64)
        info = np.empty(ROBUST_NINFO, np.float64)
        self._chk(self.L.s4p_icp_robust_sums(self.h, _fp(T), METRICS.index(metric), C.byref(r), _dp(out), _dp(info)))
        return out, info

    def refine(self, T0=None, max_iterations=30, rel_tol=1e-6, min_correspondences=3, order_source=True, metric="point",
               loss=None, trim_fraction=None, loss_scale=None, loss_c=None, info=None, gicp_epsilon=GICP_EPSILON,
               color_lambda=COLOR_LAMBDA):
        """(T float64 4x4 in the caller's frame, Result) from the start transform T0 (default identity).  metric "plane"
        minimises point-to-plane distances and needs target normals (set_target_normals or estimate_normals); metric
        "gicp" is generalized ICP (include/s4p_icp_gicp.h) with the covariance parameter gicp_epsilon in [1e-6, 1], needs
        source normals too (set_source_normals) and takes no loss; metric "symmetric" is symmetric ICP
        (include/s4p_icp_symm.h): point-to-plane along the sum of both clouds' normals, the same normals as "gicp", no
        parameter and no loss; metric "color" is coloured ICP
        (include/s4p_icp_color.h) with the geometric weight color_lambda in [0, 1], needs target normals, both intensities and
        the gradients (estimate_color_gradients) and takes no loss.  loss "trimmed" / "huber" / "tukey" refines on the
        weighted sums (include/s4p_icp_robust.h); loss=None is the plain refine.  info: an optional float64 array of 8 that
        receives the final pass's robust info."""
        _check_metric(metric, loss)
        if loss is None and (trim_fraction is not None or loss_scale is not None or loss_c is not None or info is not None):
            raise ValueError("trim_fraction / loss_scale / loss_c / info need a loss")
        rob = None if loss is None else robust_params(loss, trim_fraction, loss_scale, loss_c)
        T = np.ascontiguousarray(np.eye(4) if T0 is None else np.asarray(T0, np.float64).reshape(4, 4), np.float64).reshape(16).copy()
        p = Params()
        self.L.s4p_icp_default_params(C.byref(p))
        p.max_iterations, p.rel_tol, p.min_correspondences = int(max_iterations), float(rel_tol), int(min_correspondences)
        p.order_source = int(bool(order_source))
        r = Result()
        inf = np.zeros(ROBUST_NINFO, np.float64)
        # (function, its arguments between the parameters and T, those after the Result)
        if rob is not None:
            fn, before, after = self.L.s4p_icp_refine_robust, (METRICS.index(metric), C.byref(rob)), (_dp(inf),)
        else:
            fn, scalar = {"point": (self.L.s4p_icp_refine, ()), "plane": (self.L.s4p_icp_refine_plane, ()),
                          "gicp": (self.L.s4p_icp_refine_gicp, (gicp_epsilon,)), "symmetric": (self.L.s4p_icp_refine_symm, ()),
                          "color": (self.L.s4p_icp_refine_color, (color_lambda,))}[metric]
            before, after = tuple(float(v) for v in scalar), ()
        self._chk(fn(self.h, C.byref(p), *before, _dp(T), C.byref(r), *after))
        if rob is not None and info is not None:
            info[:] = inf
        return T.reshape(4, 4), r

    def information_sums(self, T):
        """The 11 information sums for a float T in the centred frame (layout in include/s4p_icp_info.h): n, sum d2,
        sum p', the upper triangle of sum p' p'^T over the matched target points; the context's rejection holds."""
        return self._sums(self.L.s4p_icp_information_sums, T, INFO_NSUMS)

    def information(self, T):
        """(info float64 6x6, n, rmse) of the pose T (caller frame, float64 4x4; include/s4p_icp_info.h): info = sum G^T G
        over the matched target points p, G = [-[p]x | I], rotation block first -- the weight of this pair's edge in a
        pose graph (super4pcs_amd.posegraph).  No match: zeros, 0, 0."""
        T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))
        info = np.empty(36, np.float64)
        n = C.c_int64(0)
        rmse = C.c_double(0.0)
        self._chk(self.L.s4p_icp_information(self.h, _dp(T), _dp(info), C.byref(n), C.byref(rmse)))
        return info.reshape(6, 6), int(n.value), float(rmse.value)

    def sums_batch(self, Ts, metric="point"):
        """float64 (B, 17) for "point" or (B, 31) for "plane": row b holds the bits of sums(Ts[b]) / plane_sums(Ts[b]), from
        one launch over all B float transforms in the centred frame (include/s4p_icp_batch.h)."""
        m = _batch_metric(metric)
        T = _batch_transforms(Ts, np.float32)
        B = T.shape[0]
        out = np.empty((B, PLANE_NSUMS if metric == "plane" else NSUMS), np.float64)
        self._chk(self.L.s4p_icp_sums_batch(self.h, m, B, _fp(T), _dp(out)))
        return out

    def refine_batch(self, T0s, max_iterations=30, rel_tol=1e-6, min_correspondences=3, order_source=True, metric="point"):
        """(Ts float64 (B, 4, 4) in the caller's frame, [Result] * B, order int32 (B,)) from the B start transforms T0s,
        refined side by side (include/s4p_icp_batch.h): a pose that stops leaves the launches, the final pass covers all
        B.  order[0] is the best pose: n_corr descending, then rmse ascending, then the index.  order_source=True orders
        the source once, by its image under T0s[0]."""
        m = _batch_metric(metric)
        T = _batch_transforms(T0s, np.float64)
        B = T.shape[0]
        p = BatchParams()
        self.L.s4p_icp_default_params(C.byref(p.icp))
        p.icp.max_iterations, p.icp.rel_tol, p.icp.min_correspondences = int(max_iterations), float(rel_tol), int(min_correspondences)
        p.icp.order_source = int(bool(order_source))
        p.metric = m
        res = (Result * B)()
        order = np.empty(B, np.int32)
        self._chk(self.L.s4p_icp_refine_batch(self.h, C.byref(p), B, _dp(T), res, order.ctypes.data_as(C.POINTER(C.c_int32))))
        return T, [Result.from_buffer_copy(r) for r in res], order

    def apply(self, T, X):
        """float32 (N, 3): float(T) applied to X on the device in k_apply's rounding order."""
        T = np.ascontiguousarray(np.asarray(T, np.float64).reshape(16))
        X = np.asarray(X, np.float32)
        cols = [np.ascontiguousarray(X[:, k]).copy() for k in range(3)]
        self._chk(self.L.s4p_icp_apply(self.h, _dp(T), _fp(cols[0]), _fp(cols[1]), _fp(cols[2]), X.shape[0]))
        return np.stack(cols, axis=1)


@contextlib.contextmanager
def _session(P, Q, max_distance, device, target=False, source=False, target_normals=None, normal_radius=None,
             source_normals=None, normal_k=16, rej=None):
    """One context for one convenience call, closed on every path: target P, source Q; with `target` the target normals
    (given, else estimated within normal_radius, default max_distance); with `source` the source normals (given, else the
    normal_k-nearest-neighbour normals of Q, estimated before the context is created); the rejection rej when it has a
    filter on."""
    if source and source_normals is None:
        from super4pcs_amd import normals
        source_normals = normals.estimate_normals(Q, k=normal_k)
    ctx = ICP(device)
    try:
        ctx.set_target(P, max_distance)
        ctx.set_source(Q)
        if target:
            if target_normals is not None:
                ctx.set_target_normals(target_normals)
            else:
                ctx.estimate_normals(max_distance if normal_radius is None else normal_radius)
        if source:
            ctx.set_source_normals(source_normals)
        if rej is not None and (rej.reciprocal or rej.normal_mode != NORMALS_OFF):
            ctx._chk(ctx.L.s4p_icp_set_rejection(ctx.h, C.byref(rej)))
        yield ctx
    finally:
        ctx.close()


def refine(P, Q, T0=None, max_distance=None, device=0, metric="point", target_normals=None, normal_radius=None,
           source_normals=None, normal_k=16, target_intensity=None, source_intensity=None, color_radius=None,
           reciprocal=False, normal_angle=None, normals_oriented=False, **params):
    """Convenience: one context, target P, source Q, refine from T0.  max_distance is required.  metric "plane", "gicp",
    "symmetric" and "color": the target normals are target_normals if given, else estimated within normal_radius (default max_distance).  metric
    "gicp" and "symmetric": the source normals (in Q's frame as given) are source_normals if given, else the normal_k-nearest-neighbour
    normals of Q (super4pcs_amd.normals.estimate_normals).  metric "color": target_intensity and source_intensity are
    required, one value per point as (N,), or rgb in 0..255 as (N, 3), which goes through rgb_to_intensity; the gradients are
    estimated within color_radius (default: the radius of the normals).  reciprocal / normal_angle (degrees) /
    normals_oriented set the pair rejection (ICP.set_rejection) for any metric and loss; with normal_angle, a metric that does
    not already set them gets target normals by the plane rule and source normals by the gicp rule.  params go to ICP.refine, the robust ones (loss,
    trim_fraction, loss_scale, loss_c), gicp_epsilon and color_lambda included."""
    if max_distance is None:
        raise ValueError("max_distance is required (4 * delta after a registration at delta)")
    _check_metric(metric, params.get("loss"))
    if metric == "color":
        if target_intensity is None or source_intensity is None:
            raise ValueError("metric \"color\" needs target_intensity and source_intensity")
        target_intensity, source_intensity = _as_intensity(target_intensity), _as_intensity(source_intensity)
    elif target_intensity is not None or source_intensity is not None or color_radius is not None:
        raise ValueError("target_intensity / source_intensity / color_radius need metric \"color\"")
    rej = reject_params(reciprocal, normal_angle, normals_oriented)       # validates before any device work
    by_normals = rej.normal_mode != NORMALS_OFF
    with _session(P, Q, max_distance, device, target=metric != "point" or by_normals, source=metric in NORMAL_PAIR_METRICS or by_normals,
                  target_normals=target_normals, normal_radius=normal_radius, source_normals=source_normals, normal_k=normal_k,
                  rej=rej) as ctx:                         # the rejection is set only when reciprocal or by_normals
        if metric == "color":
            ctx.set_target_intensity(target_intensity)
            ctx.set_source_intensity(source_intensity)
            r_n = max_distance if normal_radius is None else normal_radius
            ctx.estimate_color_gradients(r_n if color_radius is None else color_radius)
        return ctx.refine(T0, metric=metric, **params)


def refine_best(P, Q, T0s, max_distance=None, device=0, metric="point", target_normals=None, normal_radius=None, **params):
    """(T, Result, index): every start of T0s (B, 4, 4; 1 <= B <= 64) refined in one batch on one context (target P, source
    Q, numpy arrays or GPU torch tensors as for refine), and the one the full clouds prefer: the most correspondences, then
    the least rmse, then the first.  metric "point" or "plane" (target normals as for refine); params go to
    ICP.refine_batch.  max_distance is required."""
    if max_distance is None:
        raise ValueError("max_distance is required (4 * delta after a registration at delta)")
    _batch_metric(metric)
    T0s = _batch_transforms(T0s, np.float64)
    if metric != "plane" and (target_normals is not None or normal_radius is not None):        # refine takes them for any metric
        raise ValueError("target_normals / normal_radius need metric \"plane\"")
    with _session(P, Q, max_distance, device, target=metric == "plane", target_normals=target_normals, normal_radius=normal_radius) as ctx:
        Ts, results, order = ctx.refine_batch(T0s, metric=metric, **params)
        i = int(order[0])
        return Ts[i], results[i], i


def information_from_sums(sums, c):
    """(info 6x6, n, rmse) from the 11 information sums and the frame c (3 floats): the host half of ICP.information
    (s4p_icp_information_from_sums, no device)."""
    L = load_library()
    s = np.ascontiguousarray(sums, np.float64).reshape(INFO_NSUMS)
    c = np.ascontiguousarray(c, np.float32).reshape(3)
    info = np.empty(36, np.float64)
    n = C.c_int64(0)
    rmse = C.c_double(0.0)
    rc = L.s4p_icp_information_from_sums(_dp(s), _fp(c), _dp(info), C.byref(n), C.byref(rmse))
    if rc != 0:
        raise ICPError(rc, "information_from_sums: bad argument")
    return info.reshape(6, 6), int(n.value), float(rmse.value)


def information(P, Q, T, max_distance=None, device=0, reciprocal=False, normal_angle=None, normals_oriented=False,
                target_normals=None, normal_radius=None, source_normals=None, normal_k=16):
    """(info 6x6, n, rmse): the information matrix of the pose T (maps Q onto P, caller frame) over the pairs within
    max_distance, on one context (ICP.information).  reciprocal / normal_angle / normals_oriented set the pair rejection as
    for refine; with normal_angle the normals follow refine's rules (given, else estimated)."""
    if max_distance is None:
        raise ValueError("max_distance is required (4 * delta after a registration at delta)")
    rej = reject_params(reciprocal, normal_angle, normals_oriented)
    by_normals = rej.normal_mode != NORMALS_OFF
    with _session(P, Q, max_distance, device, target=by_normals, source=by_normals, target_normals=target_normals,
                  normal_radius=normal_radius, source_normals=source_normals, normal_k=normal_k, rej=rej) as ctx:
        return ctx.information(T)
