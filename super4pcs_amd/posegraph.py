"""ctypes binding of include/s4p_icp_posegraph.h (libsuper4pcs_icp.so): pose-graph optimisation with a line process (Choi, Zhou,
Koltun, CVPR 2015).  Host only, no device needed.

    from super4pcs_amd import posegraph
    g = posegraph.PoseGraph(poses0)                        # (N, 4, 4): world <- scan i
    g.add_edge(source=1, target=0, T=T10, info=info10)     # T maps scan 1 onto scan 0 (icp.refine's T), info from icp.information
    g.add_edge(3, 0, T30, info30, uncertain=True)          # a loop closure the line process may switch off
    poses, line, res = posegraph.optimize(g, max_distance=d)
"""
import ctypes as C

import numpy as np

MAX_NODES = 256                                            # S4P_ICP_POSEGRAPH_MAX_NODES
MAX_ITERATIONS, CONVERGED, STAGE2_SKIPPED, STALLED = 0, 1, 2, 3       # S4P_ICP_POSEGRAPH_*
STATUS_NAMES = {MAX_ITERATIONS: "max iterations", CONVERGED: "converged",
                STAGE2_SKIPPED: "stage 2 skipped: pruning would disconnect the graph",
                STALLED: "stalled: no step lowers F any further"}


class Edge(C.Structure):
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("uncertain", C.c_int32), ("reserved", C.c_int32),
                ("T", C.c_double * 16), ("info", C.c_double * 36)]


class Params(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("reference", C.c_int32), ("line_process_weight", C.c_double),
                ("prune_threshold", C.c_double), ("rel_tol", C.c_double), ("reserved", C.c_double * 3)]


class Result(C.Structure):
    _fields_ = [("iterations", C.c_int32 * 2), ("status", C.c_int32), ("n_pruned", C.c_int32), ("cost_start", C.c_double),
                ("cost_end", C.c_double), ("reserved", C.c_double * 4)]

    def as_dict(self):
        return {"iterations": [int(self.iterations[0]), int(self.iterations[1])], "status": STATUS_NAMES[self.status],
                "status_code": int(self.status), "n_pruned": int(self.n_pruned), "cost_start": self.cost_start,
                "cost_end": self.cost_end}


_DP = C.POINTER(C.c_double)
SIGNATURES = {                                             # include/s4p_icp_posegraph.h; icp.load_library declares it
    "s4p_icp_posegraph_default_params": (None, [C.POINTER(Params)]),
    "s4p_icp_posegraph_cost": (C.c_double, [C.c_int32, _DP, C.c_int32, C.POINTER(Edge), C.c_double, _DP]),
    "s4p_icp_posegraph_optimize": [C.c_int32, _DP, C.c_int32, C.POINTER(Edge), C.POINTER(Params), _DP, C.POINTER(Result)],
}

from . import icp as _icp  # noqa: E402 -- after the table: icp imports this module for it, whichever of the two comes first


class PoseGraph:
    """Nodes (N, 4, 4) float64, world <- scan i, and a list of edges (source, target, T 4x4, info 6x6, uncertain)."""

    def __init__(self, poses):
        self.poses = np.ascontiguousarray(np.asarray(poses, np.float64)).copy()
        if self.poses.ndim != 3 or self.poses.shape[1:] != (4, 4) or self.poses.shape[0] < 1:
            raise ValueError("the nodes of a pose graph are (N, 4, 4)")
        self.edges = []

    @property
    def n_nodes(self):
        return int(self.poses.shape[0])

    def add_edge(self, source, target, T, info, uncertain=False):
        T = np.asarray(T, np.float64)
        info = np.asarray(info, np.float64)
        if T.shape != (4, 4) or info.shape != (6, 6):
            raise ValueError("an edge carries a 4x4 T and a 6x6 information matrix")
        self.edges.append((int(source), int(target), T.copy(), info.copy(), bool(uncertain)))
        return len(self.edges) - 1

    def edge_array(self):
        arr = (Edge * max(len(self.edges), 1))()
        for k, (s, t, T, info, unc) in enumerate(self.edges):
            arr[k].source, arr[k].target, arr[k].uncertain, arr[k].reserved = s, t, int(unc), 0
            arr[k].T[:] = [float(v) for v in T.reshape(16)]
            arr[k].info[:] = [float(v) for v in info.reshape(36)]
        return arr


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def cost(graph, mu=0.0, return_chi2=False):
    """F of include/s4p_icp_posegraph.h at the graph's poses (mu: the line-process weight, needed with an uncertain edge);
    return_chi2: (F, chi2 per edge)."""
    L = _icp.load_library()
    poses = np.ascontiguousarray(graph.poses, np.float64)
    chi2 = np.zeros(max(len(graph.edges), 1), np.float64)
    F = L.s4p_icp_posegraph_cost(graph.n_nodes, _dp(poses), len(graph.edges), graph.edge_array(), float(mu), _dp(chi2))
    if F != F:
        raise _icp.ICPError(-1, "posegraph cost: bad argument")
    return (float(F), chi2[:len(graph.edges)]) if return_chi2 else float(F)


def default_weight(graph, max_distance, preference=1.0):
    """mu = preference * max_distance^2 * mean over the uncertain edges of info[3][3] (for icp.information's matrices the
    matched count): an uncertain edge is switched off when its matched points disagree by about max_distance on average."""
    w = [info[3, 3] for (_, _, _, info, unc) in graph.edges if unc]
    if not w:
        return 0.0
    d = float(max_distance)
    mean = 0.0
    for v in w:                                               # left to right, as the facade sums them
        mean += float(v)
    return float(preference) * (d * d) * (mean / len(w))


def optimize(graph, reference=0, line_process_weight=None, preference=1.0, max_distance=None, max_iterations=100,
             prune_threshold=0.25, rel_tol=1e-12):
    """(poses (N, 4, 4), line (n_edges,), result dict): s4p_icp_posegraph_optimize on the graph (which stays as it is).
    line_process_weight None: default_weight(graph, max_distance, preference), which needs max_distance when an edge is
    uncertain.  Raises ICPError with code -1 for what the header refuses."""
    L = _icp.load_library()
    if line_process_weight is None:
        if any(e[4] for e in graph.edges):
            if max_distance is None:
                raise ValueError("line_process_weight or max_distance is required with an uncertain edge")
            line_process_weight = default_weight(graph, max_distance, preference)
        else:
            line_process_weight = 0.0
    p = Params()
    L.s4p_icp_posegraph_default_params(C.byref(p))
    p.max_iterations, p.reference = int(max_iterations), int(reference)
    p.line_process_weight, p.prune_threshold, p.rel_tol = float(line_process_weight), float(prune_threshold), float(rel_tol)
    poses = np.ascontiguousarray(graph.poses, np.float64).copy()
    line = np.ones(max(len(graph.edges), 1), np.float64)
    r = Result()
    rc = L.s4p_icp_posegraph_optimize(graph.n_nodes, _dp(poses), len(graph.edges), graph.edge_array(), C.byref(p), _dp(line),
                                      C.byref(r))
    if rc != 0:
        raise _icp.ICPError(rc, "posegraph optimize: bad argument (include/s4p_icp_posegraph.h lists them)")
    out = r.as_dict()
    out["line_process_weight"] = float(line_process_weight)
    return poses, line[:len(graph.edges)], out
