"""Restatements for the pose-graph and information-matrix tests (include/s4p_icp_posegraph.h, include/s4p_icp_info.h): the
residual, chi2 and F in numpy / scipy, Lambda from points, graph builders, a scipy least-squares minimiser of the stated
robust cost, and the analytic windows of the multiway tests."""
import numpy as np
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation


def pose(rotvec, t):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.asarray(rotvec, np.float64)).as_matrix()
    T[:3, 3] = t
    return T


def random_pose(rng, rot_sigma, t_sigma):
    return pose(rng.normal(size=3) * rot_sigma, rng.normal(size=3) * t_sigma)


def skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]], np.float64)


def info_from_points(p):
    """Lambda = sum G^T G, G = [-[p]x | I], rotation block first."""
    p = np.asarray(p, np.float64)
    L = np.zeros((6, 6))
    S = p.sum(0)
    L[:3, :3] = (p * p).sum() * np.eye(3) - p.T @ p
    L[:3, 3:] = skew(S)
    L[3:, :3] = -skew(S)
    L[3:, 3:] = len(p) * np.eye(3)
    return L


def residual(Xs, Xt, T):
    E = np.linalg.inv(Xt) @ Xs @ np.linalg.inv(T)
    return np.concatenate([Rotation.from_matrix(E[:3, :3]).as_rotvec(), E[:3, 3]])


def chi2_all(poses, edges):
    out = []
    for (s, t, T, info, unc) in edges:
        r = residual(poses[s], poses[t], T)
        out.append(float(r @ info @ r))
    return np.array(out)


def cost(poses, edges, mu):
    c = chi2_all(poses, edges)
    F = 0.0
    for k, e in enumerate(edges):
        F += mu * c[k] / (mu + c[k]) if e[4] else c[k]
    return F, c


def line_values(poses, edges, mu):
    c = chi2_all(poses, edges)
    return np.array([(mu / (mu + c[k])) ** 2 if e[4] else 1.0 for k, e in enumerate(edges)])


def relative_error(poses, truth, reference=0):
    """max over nodes of |(X_ref^-1 X_i) - (truth_ref^-1 truth_i)| entrywise."""
    a = [np.linalg.inv(poses[reference]) @ X for X in poses]
    b = [np.linalg.inv(truth[reference]) @ X for X in truth]
    return float(max(np.max(np.abs(x - y)) for x, y in zip(a, b)))


def scipy_minimise(poses0, edges, mu, reference=0):
    """The minimiser of the stated F over the poses (reference fixed) by scipy.optimize.least_squares on the residuals
    sqrt(rho_e) split through the Cholesky factor of Lambda_e: sum of squares = F exactly.  Returns (poses, F)."""
    N = len(poses0)
    free = [i for i in range(N) if i != reference]
    chol = [np.linalg.cholesky(e[3]).T for e in edges]          # info = U^T U

    def unpack(x):
        P = [None] * N
        P[reference] = poses0[reference]
        for k, i in enumerate(free):
            P[i] = poses0[i] @ pose(x[6 * k:6 * k + 3], x[6 * k + 3:6 * k + 6])
        return P

    def fun(x):
        P = unpack(x)
        out = []
        for (s, t, T, info, unc), U in zip(edges, chol):
            y = U @ residual(P[s], P[t], T)
            if unc:
                c = float(y @ y)
                y = y * np.sqrt(mu / (mu + c))
            out.append(y)
        return np.concatenate(out)

    x = np.zeros(6 * len(free))
    for _ in range(3):                                           # restarts tighten the tolerances' last digits
        r = least_squares(fun, x, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, x_scale=1.0, max_nfev=2000)
        x = r.x
    P = unpack(x)
    return np.array(P), float(np.sum(fun(x) ** 2))


def consistent_graph(rng, n_nodes, extra_edges=4, rot_sigma=0.5, t_sigma=1.0):
    """True poses, a chain (i, i - 1) plus extra_edges random pairs, each with T from the truth and a random SPD Lambda."""
    truth = np.array([random_pose(rng, rot_sigma, t_sigma) for _ in range(n_nodes)])
    pairs = [(i, i - 1) for i in range(1, n_nodes)]
    want = min(n_nodes - 1 + extra_edges, n_nodes * (n_nodes - 1) // 2)
    while len(pairs) < want:
        s, t = (int(v) for v in rng.choice(n_nodes, 2, replace=False))
        if (s, t) not in pairs and (t, s) not in pairs:
            pairs.append((s, t))
    edges = []
    for (s, t) in pairs:
        A = rng.normal(size=(6, 6))
        info = A @ A.T + 6 * np.eye(6)
        edges.append((s, t, np.linalg.inv(truth[t]) @ truth[s], 0.5 * (info + info.T), False))
    return truth, edges


def loop_scenario(seed=0):
    """The six-node loop of the pose-graph tests: noisy odometry edges (s, s - 1), four noisy true closures, one false
    closure (4, 0).  Returns (truth, start = the odometry chain, edges, mu, index of the false edge)."""
    rng = np.random.default_rng(seed)
    N, d = 6, 0.05
    truth = np.array([random_pose(rng, 0.5, 1.0) for _ in range(N)])

    def measured(s, t, npts):
        T = np.linalg.inv(truth[t]) @ truth[s] @ random_pose(rng, 0.004, 0.004)
        return T, info_from_points(rng.uniform(-1, 1, size=(npts, 3)))

    edges = []
    for s in range(1, N):
        T, info = measured(s, s - 1, 400)
        edges.append((s, s - 1, T, info, False))
    for (s, t) in ((5, 0), (3, 0), (4, 1), (5, 2)):
        T, info = measured(s, t, 300)
        edges.append((s, t, T, info, True))
    T, info = measured(4, 0, 300)
    edges.append((4, 0, T @ pose([0, 0, np.radians(30.0)], [0.3, 0, 0]), info, True))
    mu = 1.0 * d * d * float(np.mean([e[3][3, 3] for e in edges if e[4]]))
    start = [truth[0]]
    for s in range(1, N):
        start.append(start[s - 1] @ edges[s - 1][2])            # X_s = X_{s-1} T_{s -> s-1}
    return truth, np.array(start), edges, mu, len(edges) - 1


# ---------------------------------------------------------------------------------------------------------------------
# the multiway scene: overlapping windows of one analytic bumpy surface

def surface(xy):
    x, y = xy[:, 0], xy[:, 1]
    return 0.15 * np.sin(2.3 * x) * np.cos(1.7 * y) + 0.08 * np.sin(5.1 * x + 0.4) + 0.07 * np.cos(4.3 * y - 0.9) + 0.05 * x * y


def windows(n_windows=5, n_points=3000, width=1.0, radius=0.45, seed=5):
    """(clouds in their own frames float32, truth (n, 4, 4) world <- scan i).  Window i is the square of edge w about the
    i-th of n_windows points on a circle of the given radius: a ring in which every window shares 0.39 to 0.47 of its area
    with the next one, the last with the first (the loop closure), and 0.14 to 0.15 with its second neighbours.  Scan i =
    truth_i^-1 applied to its world points."""
    rng = np.random.default_rng(seed)
    clouds, truth = [], []
    for i in range(n_windows):
        a = 2.0 * np.pi * i / n_windows
        c = np.array([radius * np.cos(a), radius * np.sin(a)])
        xy = rng.uniform(c - 0.5 * width, c + 0.5 * width, size=(n_points, 2))
        W = np.concatenate([xy, surface(xy)[:, None]], 1)
        X = pose(rng.normal(size=3) * 0.3, rng.normal(size=3) * 0.5) if i else np.eye(4)
        Xi = np.linalg.inv(X)
        clouds.append((W @ Xi[:3, :3].T + Xi[:3, 3]).astype(np.float32))
        truth.append(X)
    return clouds, np.array(truth)


def perturbed(truth, rot_deg, t, seed=9):
    rng = np.random.default_rng(seed)
    out = []
    for X in truth:
        a = rng.normal(size=3); a *= np.radians(rot_deg) / np.linalg.norm(a)
        b = rng.normal(size=3); b *= t / np.linalg.norm(b)
        out.append(X @ pose(a, b))
    return np.array(out)


def pose_error(X, truth):
    """(rotation error in radians, translation error) of X against truth."""
    E = np.linalg.inv(truth) @ X
    return float(np.linalg.norm(Rotation.from_matrix(E[:3, :3]).as_rotvec())), float(np.linalg.norm(E[:3, 3]))


def cloud_error(X, X_true, cloud):
    """RMS over the cloud's points of |X p - X_true p|: a pose error in the cloud's own units."""
    p = np.asarray(cloud, np.float64)
    a = p @ X[:3, :3].T + X[:3, 3]
    b = p @ X_true[:3, :3].T + X_true[:3, 3]
    return float(np.sqrt(((a - b) ** 2).sum(1).mean()))
