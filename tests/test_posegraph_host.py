"""Pose-graph optimisation (include/s4p_icp_posegraph.h) on the host, no device: the cost against a numpy restatement, a
consistent graph, the loop scenario with a false closure against scipy, pruning, the skipped stage 2, the refusals and the
node limit.  Restatements: tests/posegraph_helpers.py."""
import numpy as np
import pytest

from tests import posegraph_helpers as H


@pytest.fixture(scope="module")
def PG(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import posegraph
    return posegraph


def _graph(PG, poses, edges):
    g = PG.PoseGraph(poses)
    for e in edges:
        g.add_edge(*e)
    return g


def _noisy_graph(rng, n_nodes, n_uncertain):
    truth, edges = H.consistent_graph(rng, n_nodes, extra_edges=n_uncertain)
    edges = [(s, t, T @ H.random_pose(rng, 0.05, 0.05), info, k >= n_nodes - 1) for k, (s, t, T, info, _) in enumerate(edges)]
    poses = np.array([X @ H.random_pose(rng, 0.1, 0.1) for X in truth])
    return poses, edges


def test_cost_equals_the_numpy_restatement(PG):
    rng = np.random.default_rng(21)
    worst = 0.0
    for k in range(20):
        n = int(rng.integers(2, 12))
        poses, edges = _noisy_graph(rng, n, int(rng.integers(0, 5)))
        mu = float(10.0 ** rng.uniform(-2, 2))
        F, chi2 = PG.cost(_graph(PG, poses, edges), mu, return_chi2=True)
        Fn, cn = H.cost(poses, edges, mu)
        worst = max(worst, abs(F - Fn) / Fn, float(np.max(np.abs(chi2 - cn) / cn)))
    print("cost: worst relative difference to numpy %.3g" % worst)
    assert worst <= 1e-12


def test_consistent_graph_returns_to_the_true_relative_poses(PG):
    rng = np.random.default_rng(1)
    for n in (2, 3, 8, 17):
        truth, edges = H.consistent_graph(rng, n)
        start = []
        for X in truth:
            a = rng.normal(size=3); a *= rng.uniform(0, np.radians(10.0)) / np.linalg.norm(a)
            b = rng.normal(size=3); b *= rng.uniform(0, 0.5) / np.linalg.norm(b)
            start.append(X @ H.pose(a, b))
        start = np.array(start)
        ref = int(rng.integers(0, n))
        poses, line, res = PG.optimize(_graph(PG, start, edges), reference=ref)
        err = H.relative_error(poses, truth, ref)
        print("consistent graph, %d nodes, reference %d: %s, relative pose error %.3g" % (n, ref, res, err))
        assert err <= 1e-9
        assert res["cost_end"] <= 1e-18 * res["cost_start"]
        assert poses[ref].tobytes() == start[ref].tobytes()
        assert np.all(line == 1.0) and res["n_pruned"] == 0 and res["iterations"][1] == 0


@pytest.fixture(scope="module")
def loop(PG):
    truth, start, edges, mu, false_edge = H.loop_scenario(5)
    Ps, Fs = H.scipy_minimise(start, edges, mu)
    return {"truth": truth, "start": start, "edges": edges, "mu": mu, "false": false_edge, "scipy_poses": Ps, "scipy_F": Fs}


def test_loop_scenario_prunes_the_false_closure_and_meets_scipys_minimum(PG, loop):
    """Six nodes, noisy odometry, four true closures and one false one (30 degrees, 0.3 off), mu = 0.75 by the default
    rule, start = the odometry chain.  Stage 1 (prune_threshold 0 keeps every edge) against scipy.optimize.least_squares
    on the stated robust cost: F <= scipy's (1 + 1e-9), poses within 1e-5; then the default call prunes the false edge
    and no other."""
    edges, mu, kf = loop["edges"], loop["mu"], loop["false"]
    assert abs(mu - 0.75) <= 1e-12
    g = _graph(PG, loop["start"], edges)
    assert abs(PG.default_weight(g, 0.05) - mu) <= 1e-15
    l_scipy = H.line_values(loop["scipy_poses"], edges, mu)
    assert l_scipy[kf] <= 1e-3 and np.all(np.delete(l_scipy, kf) >= 0.25), l_scipy
    p1, l1, r1 = PG.optimize(g, max_distance=0.05, prune_threshold=0.0)
    F1 = H.cost(p1, edges, mu)[0]
    dpose = float(np.max(np.abs(p1 - loop["scipy_poses"])))
    print("loop: scipy F %.17g, library stage 1 F %.17g (its own %.17g), relative difference %.3g, pose difference %.3g, iterations %s"
          % (loop["scipy_F"], F1, r1["cost_end"], (F1 - loop["scipy_F"]) / loop["scipy_F"], dpose, r1["iterations"]))
    print("loop: line values, library %s, scipy %s" % (np.array2string(l1, precision=5), np.array2string(l_scipy, precision=5)))
    assert r1["n_pruned"] == 0 and r1["status_code"] == PG.CONVERGED
    assert F1 <= loop["scipy_F"] * (1 + 1e-9)
    assert abs(r1["cost_end"] - F1) <= 1e-12 * F1
    assert dpose <= 1e-5
    poses, line, res = PG.optimize(g, max_distance=0.05)
    pruned = [k for k in range(len(edges)) if line[k] < 0.25]
    assert pruned == [kf] and res["n_pruned"] == 1 and res["iterations"][1] > 0 and res["status_code"] == PG.CONVERGED
    assert res["cost_end"] <= res["cost_start"]
    assert np.array_equal(g.poses, loop["start"])                    # the graph stays as it was


def test_pruning_equals_optimising_without_the_false_edge(PG, loop):
    edges, kf = loop["edges"], loop["false"]
    poses, line, res = PG.optimize(_graph(PG, loop["start"], edges), line_process_weight=loop["mu"])
    kept = [e for k, e in enumerate(edges) if k != kf]
    p2, l2, r2 = PG.optimize(_graph(PG, loop["start"], kept), line_process_weight=loop["mu"])
    d = float(np.max(np.abs(poses - p2)))
    print("stage 2 against the graph without the false edge: pose difference %.3g, costs %.17g %.17g" % (d, res["cost_end"], r2["cost_end"]))
    assert r2["n_pruned"] == 0
    assert d <= 1e-9
    assert np.max(np.abs(np.delete(line, kf) - l2)) <= 1e-9


def test_stage_two_is_skipped_when_pruning_would_disconnect(PG):
    """The false closure is node 3's only link: its line value is below the threshold, dropping it would cut node 3 off,
    and the status says that stage 2 was skipped.  A node's only link can always be satisfied by moving the node, so an
    optimised stage 1 ends with l = 1 on it; the line values judged here are those of the given poses (max_iterations 0)."""
    rng = np.random.default_rng(8)
    truth, edges = H.consistent_graph(rng, 4, extra_edges=0)
    info = H.info_from_points(rng.uniform(-1, 1, size=(300, 3)))
    edges = [(s, t, T, info, False) for (s, t, T, _, _) in edges[:2]]               # 1-0, 2-1
    edges.append((2, 0, np.linalg.inv(truth[0]) @ truth[2], info, True))
    edges.append((3, 0, H.pose([0, 0, 0.5], [0.3, 0, 0]) @ np.linalg.inv(truth[0]) @ truth[3], info, True))
    start = truth.copy()
    g = _graph(PG, start, edges)
    poses, line, res = PG.optimize(g, line_process_weight=1e-3, max_iterations=0)
    print("only link:", res, line)
    assert np.array_equal(poses, start)
    full = PG.optimize(g, line_process_weight=1e-3)
    assert full[2]["n_pruned"] == 0 and full[1][3] >= 0.25                          # optimised: the link is satisfied
    assert res["status_code"] == PG.STAGE2_SKIPPED and res["n_pruned"] == 1 and res["iterations"][1] == 0
    assert line[3] < 0.25 and np.all(line[:3] >= 0.25)
    assert "skipped" in res["status"]


def _refusals(truth, edges):
    s, t, T, info, unc = edges[0]
    bad_T = T.copy(); bad_T[1, 2] = np.nan
    bad_info = info.copy(); bad_info[2, 3] = np.inf
    skewed = info.copy(); skewed[0, 5] += 1e-8 * np.max(np.abs(info))
    lone = [e for e in edges if 3 not in (e[0], e[1])]
    return {
        "node not connected": (truth, lone, {}),
        "index out of range": (truth, [(len(truth), t, T, info, unc)] + edges[1:], {}),
        "negative index": (truth, [(s, -1, T, info, unc)] + edges[1:], {}),
        "source equals target": (truth, edges + [(2, 2, T, info, False)], {}),
        "non-finite T": (truth, [(s, t, bad_T, info, unc)] + edges[1:], {}),
        "non-finite information": (truth, [(s, t, T, bad_info, unc)] + edges[1:], {}),
        "asymmetric information": (truth, [(s, t, T, skewed, unc)] + edges[1:], {}),
        "mu zero with an uncertain edge": (truth, edges + [(3, 0, T, info, True)], {"line_process_weight": 0.0}),
        "mu negative with an uncertain edge": (truth, edges + [(3, 0, T, info, True)], {"line_process_weight": -1.0}),
        "reference out of range": (truth, edges, {"reference": len(truth)}),
    }


def test_refusals_return_bad_arg_and_leave_the_poses(PG):
    import ctypes as C
    from super4pcs_amd import icp
    rng = np.random.default_rng(3)
    truth, edges = H.consistent_graph(rng, 5)
    cases = _refusals(truth, edges)
    nan_pose = truth.copy(); nan_pose[2, 0, 3] = np.nan
    cases["non-finite pose"] = (nan_pose, edges, {})
    L = icp.load_library()
    for name, (poses, ed, kw) in cases.items():
        g = _graph(PG, poses, ed)
        with pytest.raises(icp.ICPError) as e:
            PG.optimize(g, **kw)
        assert e.value.code == -1, name
        # the C entry point itself: -1 and the caller's buffer untouched
        p = PG.Params()
        L.s4p_icp_posegraph_default_params(C.byref(p))
        p.line_process_weight = kw.get("line_process_weight", 1.0)
        p.reference = kw.get("reference", 0)
        buf = np.ascontiguousarray(poses, np.float64).copy()
        before = buf.tobytes()
        rc = L.s4p_icp_posegraph_optimize(len(poses), buf.ctypes.data_as(C.POINTER(C.c_double)), len(ed), g.edge_array(), C.byref(p), None, None)
        assert rc == -1 and buf.tobytes() == before, name
    # an asymmetry below 1e-9 of the largest entry is accepted
    s, t, T, info, unc = edges[0]
    ok = info.copy(); ok[0, 5] += 1e-11 * np.max(np.abs(info))
    PG.optimize(_graph(PG, truth, [(s, t, T, ok, unc)] + edges[1:]))


def test_node_limit(PG):
    """256 nodes run (a chain with a few closures; the dense system is 1530 x 1530), 257 are refused."""
    from super4pcs_amd import icp
    rng = np.random.default_rng(6)
    truth, edges = H.consistent_graph(rng, 257, extra_edges=0, rot_sigma=0.2)
    edges256 = [e for e in edges if e[0] < 256 and e[1] < 256]
    edges256.append((255, 0, np.linalg.inv(truth[0]) @ truth[255], edges[0][3], False))
    start = np.array([X @ H.random_pose(rng, 0.01, 0.01) for X in truth[:256]])
    poses, line, res = PG.optimize(_graph(PG, start, edges256), max_iterations=4)
    print("256 nodes:", res, "relative pose error", H.relative_error(poses, truth[:256]))
    assert res["cost_end"] <= 1e-6 * res["cost_start"]
    assert poses[0].tobytes() == start[0].tobytes()
    with pytest.raises(icp.ICPError) as e:
        PG.optimize(_graph(PG, truth, edges))
    assert e.value.code == -1
    assert PG.MAX_NODES == 256
