"""Multi-scale (coarse-to-fine) ICP as a composition of voxel.voxel_downsample and icp.refine.

    from super4pcs_amd import multiscale
    T, levels = multiscale.refine_multiscale(P, Q, T0, voxel_sizes=(0.04, 0.01, 0), max_distance=0.008)

A large correspondence distance widens ICP's basin but is expensive on the full-resolution target, whose grid edge follows
it; here the large distances run on voxel-downsampled pairs, and the full-resolution level starts from a pose that is
already close.  Nothing is added to the ICP library: level l is exactly one icp.refine call on the level's clouds.
"""
import numpy as np

from . import icp as _icp
from . import voxel as _voxel

DISTANCE_FACTOR = 3.0          # default d_l = max(d, 3 * v_l): common practice, not measured here
DEFAULT_ITERATIONS = 30


def _per_level(name, value, default, nl):
    if value is None:
        return [default] * nl
    if np.ndim(value) == 0:
        return [value] * nl
    value = list(value)
    if len(value) != nl:
        raise ValueError("%s has %d entries for %d levels" % (name, len(value), nl))
    return value


def level_plan(voxel_sizes, max_distances=None, max_iterations=None, max_distance=None):
    """[(voxel size (0.0: the clouds as given), max_distance, max_iterations)] per level, coarse to fine, checked."""
    if voxel_sizes is None or np.ndim(voxel_sizes) != 1 or len(voxel_sizes) == 0:
        raise ValueError("voxel_sizes is a non-empty sequence, coarse to fine (0 or None: the clouds as given)")
    sizes = [0.0 if v is None else float(v) for v in voxel_sizes]
    for v in sizes:
        if not (np.isfinite(v) and v >= 0):
            raise ValueError("voxel sizes are finite and >= 0, got %r" % v)
    for a, b in zip(sizes, sizes[1:]):
        if b > a:
            raise ValueError("voxel_sizes must be non-increasing (coarse to fine, 0 counted as smallest), got %r" % (sizes,))
    nl = len(sizes)
    if max_distances is None:
        if max_distance is None:
            raise ValueError("max_distances=None needs max_distance= (then d_l = max(max_distance, 3 * voxel_size_l))")
        d = float(max_distance)
        dists = [max(d, DISTANCE_FACTOR * v) for v in sizes]
    else:
        if max_distance is not None:
            raise ValueError("give max_distances (per level) or max_distance (the finest), not both")
        dists = [float(d) for d in _per_level("max_distances", max_distances, None, nl)]
    its = [int(i) for i in _per_level("max_iterations", max_iterations, DEFAULT_ITERATIONS, nl)]
    return list(zip(sizes, dists, its))


def _level_cloud(X, v, normals, intensity, device):
    """(cloud, normals, intensity) of one level: voxel means at v > 0 (normals renormalised), the inputs themselves at 0."""
    if v == 0.0:
        return X, normals, intensity
    xyz, inten, nrm, _, _ = _voxel.voxel_downsample(X, v, attrs=intensity, normals=normals, device=device)
    return xyz, nrm, inten


_BATCH_PARAMS = ("rel_tol", "min_correspondences", "order_source", "normal_radius")


def refine_multiscale(P, Q, T0=None, voxel_sizes=(0,), max_distances=None, max_iterations=None, device=0, metric="point",
                      target_normals=None, source_normals=None, target_intensity=None, source_intensity=None, starts=None,
                      **params):
    """Coarse-to-fine ICP: (T float64 4x4, [icp.Result per level]).

    Levels run in the order given.  voxel_sizes[l] > 0 downsamples both clouds at that size (voxel.voxel_downsample; Q in its
    own frame, not after applying T), 0 or None takes the clouds as given; sizes must be non-increasing with 0 counted as
    smallest.  Level l is exactly icp.refine(P_l, Q_l, T0=T_{l-1}, max_distance=d_l, max_iterations=it_l, metric=metric,
    **params) with the level's attributes in place of the caller's: given normals are voxel means, renormalised; given
    intensities are voxel means (rgb goes through icp.rgb_to_intensity first); normals not given follow icp.refine's own rule
    on the level's clouds.  Every metric and loss of icp.refine works, with the same refusals.

    max_distances: one distance per level.  max_distances=None needs max_distance= (d); then d_l = max(d, 3 * v_l).  The factor
    3 follows common practice (level distances of about three voxels); it is not measured here.  max_iterations: one count
    per level, or one number for all; None is 30 per level.

    starts: B start transforms (B, 4, 4) in place of T0.  The coarsest level is then one icp.refine_best on the level's
    clouds (every start refined side by side, ranked by correspondences, then rmse), and its best pose feeds the remaining
    levels unchanged; results[0] is that pose's Result.  Only the metrics "point" and "plane" without a loss and without pair
    rejection have a batch form: anything else with starts= raises ValueError."""
    if starts is not None:
        if T0 is not None:
            raise ValueError("give T0 (one start) or starts (several), not both")
        if metric not in _icp.METRICS or params.get("loss") is not None:
            raise ValueError("starts= needs metric \"point\" or \"plane\" and no loss (robust losses, \"gicp\", \"symmetric\" and \"color\" have no batch form)")
        if params.get("reciprocal") or params.get("normal_angle") is not None:
            raise ValueError("starts= takes no pair rejection (the batch has no split pass)")
        starts = _icp._batch_transforms(starts, np.float64)
    plan = level_plan(voxel_sizes, max_distances, max_iterations, params.pop("max_distance", None))
    _icp._check_metric(metric, params.get("loss"))
    if target_intensity is not None:
        target_intensity = _icp._as_intensity(target_intensity)
    if source_intensity is not None:
        source_intensity = _icp._as_intensity(source_intensity)
    T = None if T0 is None else np.asarray(T0, np.float64).reshape(4, 4)
    results = []
    cache = {}
    for v, d, it in plan:
        if v not in cache:
            cache = {v: (_level_cloud(P, v, target_normals, target_intensity, device),
                         _level_cloud(Q, v, source_normals, source_intensity, device))}
        (Pl, Pn, Pi), (Ql, Qn, Qi) = cache[v]
        if starts is not None and not results:
            T, r, _ = _icp.refine_best(Pl, Ql, starts, max_distance=d, device=device, metric=metric,
                                       target_normals=Pn if metric == "plane" else None, max_iterations=it,
                                       **{k: params[k] for k in _BATCH_PARAMS if k in params and (k != "normal_radius" or metric == "plane")})
            results.append(r)
            continue
        T, r = _icp.refine(Pl, Ql, T0=T, max_distance=d, device=device, metric=metric, target_normals=Pn, source_normals=Qn,
                           target_intensity=Pi, source_intensity=Qi, max_iterations=it, **params)
        results.append(r)
    return T, results
