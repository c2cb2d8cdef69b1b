"""Multiway registration: N scans into one frame.  Pairwise ICP on the device (super4pcs_amd.icp) gives a pose and its
information matrix per pair of scans; a pose graph with a line process (super4pcs_amd.posegraph) reconciles them and switches
off the pairs that contradict the rest.  DESIGN.md section "Multiway registration".

    from super4pcs_amd import multiway
    poses, graph, report = multiway.register_multiway(clouds, poses0, max_distance=4 * delta)
    # poses[i] maps scan i into the frame of scan 0 (world <- scan i); report["edges"][k]: n, rmse, fitness, l of edge k

poses0 come from the caller's pairwise runs (a global registration per pair is not made here).
"""
import numpy as np

from . import icp as _icp
from . import posegraph as _pg

NORMAL_METRICS = ("plane", "gicp", "symmetric")            # the metrics that need target normals
METRICS = ("point",) + NORMAL_METRICS                      # "color" needs intensities, which a list of clouds does not carry


def _inverse(X):
    """The rigid inverse [R^T | -R^T t], term by term as the facade (algorithms/multiway.h) forms it."""
    out = np.eye(4)
    for r in range(3):
        for c in range(3):
            out[r, c] = X[c, r]
        out[r, 3] = -((float(X[0, r]) * float(X[0, 3]) + float(X[1, r]) * float(X[1, 3])) + float(X[2, r]) * float(X[2, 3]))
    return out


def default_pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def register_multiway(clouds, poses0=None, max_distance=None, pairs=None, metric="plane", min_fitness=0.3, device=0,
                      normal_radius=None, normal_k=16, reference=0, line_process_weight=None, preference=1.0,
                      graph_iterations=100, prune_threshold=0.25, min_correspondences=3, **icp_kwargs):
    """(poses (N, 4, 4), graph, report).  clouds: N (n_i, 3) float32 numpy arrays or GPU torch tensors; poses0: (N, 4, 4)
    world <- scan i (None: identities); pairs: (i, j) with i < j (None: all).  For each target i (one set_target, plus
    normals estimated within normal_radius, default max_distance, when the metric needs them) and each source j > i of the
    pairs: set_source, ICP.refine from poses0[i]^-1 poses0[j] with icp_kwargs, ICP.information at the refined pose.
    j == i + 1 gives a certain edge (fewer than min_correspondences matches, which also goes to refine: ICPError); any other pair an uncertain edge
    when its fitness >= min_fitness and no edge below.  Then posegraph.optimize from poses0 (line_process_weight None:
    posegraph.default_weight with max_distance and preference).  report: {"edges": [{source, target, uncertain, n, rmse,
    fitness, l}], "dropped": [(i, j, fitness)], "optimize": posegraph's result dict}."""
    if max_distance is None:
        raise ValueError("max_distance is required (4 * delta after registrations at delta)")
    if metric not in METRICS:
        raise ValueError("metric must be one of %s" % (METRICS,))
    N = len(clouds)
    if N < 2:
        raise ValueError("multiway registration needs at least two clouds")
    if N > _pg.MAX_NODES:
        raise ValueError("at most %d clouds" % _pg.MAX_NODES)
    poses0 = np.tile(np.eye(4), (N, 1, 1)) if poses0 is None else np.ascontiguousarray(np.asarray(poses0, np.float64))
    if poses0.shape != (N, 4, 4):
        raise ValueError("poses0 is (N, 4, 4)")
    pairs = default_pairs(N) if pairs is None else [(int(i), int(j)) for (i, j) in pairs]
    for (i, j) in pairs:
        if not (0 <= i < j < N):
            raise ValueError("pairs are (i, j) with 0 <= i < j < N")
    for i in range(N - 1):
        if (i, i + 1) not in pairs:
            raise ValueError("pairs must hold every (i, i + 1): the certain edges connect the graph")
    min_corr = int(min_correspondences)
    src_normals = {}
    if metric in _icp.NORMAL_PAIR_METRICS:
        from . import normals
        for j in sorted({j for (_, j) in pairs}):
            src_normals[j] = normals.estimate_normals(clouds[j], k=normal_k)
    graph = _pg.PoseGraph(poses0)
    edges, dropped = [], []
    ctx = _icp.ICP(device)
    try:
        for i in range(N - 1):
            sources = sorted(j for (a, j) in pairs if a == i)
            if not sources:
                continue
            ctx.set_target(clouds[i], max_distance)
            if metric in NORMAL_METRICS:
                ctx.estimate_normals(max_distance if normal_radius is None else normal_radius)
            Xi_inv = _inverse(poses0[i])
            for j in sources:
                ctx.set_source(clouds[j])
                if metric in _icp.NORMAL_PAIR_METRICS:
                    ctx.set_source_normals(src_normals[j])
                T, res = ctx.refine(_icp.compose(Xi_inv, poses0[j]), metric=metric, min_correspondences=min_corr, **icp_kwargs)
                info, n, rmse = ctx.information(T)
                certain = j == i + 1
                if certain and n < max(min_corr, 1):
                    raise _icp.ICPError(-1, "register_multiway: scans %d and %d share %d correspondences (fewer than %d)"
                                        % (i, j, n, max(min_corr, 1)))
                if not certain and not (res.fitness >= min_fitness and n >= 1):
                    dropped.append((i, j, float(res.fitness)))
                    continue
                graph.add_edge(j, i, T, info, uncertain=not certain)
                edges.append({"source": j, "target": i, "uncertain": not certain, "n": n, "rmse": rmse,
                              "fitness": float(res.fitness)})
    finally:
        ctx.close()
    poses, line, result = _pg.optimize(graph, reference=reference, line_process_weight=line_process_weight, preference=preference,
                                       max_distance=max_distance, max_iterations=graph_iterations, prune_threshold=prune_threshold)
    for e, l in zip(edges, line):
        e["l"] = float(l)
    return poses, graph, {"edges": edges, "dropped": dropped, "optimize": result}
