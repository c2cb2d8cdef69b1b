"""What the multi-scale ICP tests share: the small pair of the composition tests with its attributes, the reduced-scale
lidar pair of the basin test, start poses and the pose error."""
import numpy as np

from tests import apps


def rot_about(axis, deg, centre):
    """4x4: a rotation by deg degrees about the axis through centre."""
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = np.asarray(centre, np.float64) - T[:3, :3] @ np.asarray(centre, np.float64)
    return T


def pose_error(T, T_gt, Q):
    """Root mean square distance between the points of Q under T and under T_gt."""
    Q = np.asarray(Q, np.float64)
    D = np.asarray(T, np.float64) - np.asarray(T_gt, np.float64)
    d = Q @ D[:3, :3].T + D[:3, 3]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def small_pair(n=6000, seed=12):
    """A bumpy pair of a few thousand points with unit normals, intensities and a start 1.5 degrees off the truth."""
    from super4pcs_amd import datasets as D
    from tests import icp_color_helpers as CH
    P, Q, T_gt = D.bumpy_pair(n, overlap=0.7, delta=0.004, seed=seed)
    rng = np.random.default_rng(seed)

    def unit(X):
        N = X.astype(np.float64) + 0.05 * rng.normal(size=X.shape)         # roughly radial: the clouds are bumpy spheres
        return (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)

    Pw = (Q.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3])
    case = {"P": P, "Q": Q, "T_gt": T_gt, "Np": unit(P), "Ip": CH.texture(P, 3.0), "Iq": CH.texture(Pw, 3.0)}
    Nq_world = unit(Pw.astype(np.float32))
    case["Nq"] = (Nq_world.astype(np.float64) @ T_gt[:3, :3]).astype(np.float32)      # in Q's own frame
    case["T0"] = T_gt @ rot_about((0.3, -0.5, 0.8), 1.5, Q.astype(np.float64).mean(0))
    return case


BASIN_DELTA = 0.05
BASIN_D = 4 * BASIN_DELTA                      # the finest level's distance, as the registration tests use it
BASIN_VOXELS = (0.4, 0.15, 0.0)
BASIN_ITERATIONS = 30                          # per level; the single-level run gets the same total
BASIN_AXIS = (0.3, -0.5, 0.8)
BASIN_START_DEG = 20.0                         # found on the device: see DESIGN.md section 19


def basin_pair():
    """The reduced-scale lidar pair of tests/test_gpu_icp.py: 100 000 returns per scan, known pose."""
    from super4pcs_amd import datasets as D
    return D.lidar_pair_scaled(0.02, delta=BASIN_DELTA)


def basin_start(T_gt, Q, deg):
    return T_gt @ rot_about(BASIN_AXIS, deg, np.asarray(Q, np.float64).mean(0))


def build_app(outdir, extra=()):
    """tests/icp_multiscale_app/main.cpp against the facade headers, libsuper4pcs_icp.so and libsuper4pcs_normals.so."""
    return apps.build_app(outdir, "icp_multiscale_app", ("super4pcs_icp", "super4pcs_normals", "dl"), ("-Werror",) + tuple(extra))


move = apps.move_f32


def facade_chain(icp, voxel, P, Q, T0, levels, **kw):
    """RefineICPMultiScale's order of operations restated on the Python binding: per level (voxel, distance, iterations) both
    clouds downsampled (Q in its own frame), Q's copy moved by the float pose, icp.refine from the identity, pose <-
    float(dT * pose); then Q moved once.  Returns (float32 pose, [Result], moved Q)."""
    T = np.asarray(T0, np.float32).reshape(4, 4)
    results = []
    for v, d, it in levels:
        Pl = voxel.voxel_downsample(P, v)[0] if v > 0 else P
        Ql = voxel.voxel_downsample(Q, v)[0] if v > 0 else Q
        dT, r = icp.refine(Pl, move(T, Ql), T0=np.eye(4), max_distance=d, max_iterations=it, **kw)
        T = icp.compose(dT, T.astype(np.float64)).astype(np.float32)
        results.append(r)
    return T, results, move(T, Q)
