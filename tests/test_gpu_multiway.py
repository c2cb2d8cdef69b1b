"""Multiway registration on the MI355X (super4pcs_amd.multiway): register_multiway against its own chain of ICP.refine,
ICP.information and posegraph.optimize calls, the edge rules, and the accuracy of the optimised poses against the chain of
the certain edges on a ring of five overlapping windows of one analytic surface."""
import os
import subprocess

import numpy as np
import pytest

from tests import apps
from tests import posegraph_helpers as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
D = 0.06                                   # max_distance: about three point spacings of the 3000-point unit windows
MIN_FITNESS = 0.35                         # ring neighbours share 0.39 to 0.47 of their area, second neighbours 0.15
# The optimised poses may be worse than the chain's at single nodes; over all nodes their RMS error may exceed the chain's
# by this much (cloud units).  Chosen after the first run, whose values (identical from run to run) are in DESIGN.md 25.
ACCURACY_MARGIN = 1.0e-4


@pytest.fixture(scope="module")
def mods(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    B.build_normals()
    from super4pcs_amd import icp, multiway, posegraph
    return icp, multiway, posegraph


@pytest.fixture(scope="module")
def scene():
    clouds, truth = PH.windows()
    return clouds, truth, PH.perturbed(truth, 1.5, 0.5 * D)


@pytest.fixture(scope="module")
def registered(mods, scene):
    icp, multiway, posegraph = mods
    clouds, truth, poses0 = scene
    return multiway.register_multiway(clouds, poses0, max_distance=D, min_fitness=MIN_FITNESS)


def _inv(X):
    from super4pcs_amd import multiway
    return multiway._inverse(X)                  # [R^T | -R^T t] term by term, the one order the Python and the facade share


def test_register_multiway_is_its_own_chain_of_calls(mods, scene, registered):
    icp, multiway, posegraph = mods
    clouds, truth, poses0 = scene
    poses, graph, report = registered
    N = len(clouds)
    g = posegraph.PoseGraph(poses0)
    rows = []
    ctx = icp.ICP(0)
    for i in range(N - 1):
        ctx.set_target(clouds[i], D)
        ctx.estimate_normals(D)
        for j in range(i + 1, N):
            ctx.set_source(clouds[j])
            T, res = ctx.refine(icp.compose(_inv(poses0[i]), poses0[j]), metric="plane")
            info, n, rmse = ctx.information(T)
            if j == i + 1 or res.fitness >= MIN_FITNESS:
                g.add_edge(j, i, T, info, uncertain=j != i + 1)
                rows.append((j, i, n, rmse, res.fitness))
    ctx.close()
    want, line, result = posegraph.optimize(g, max_distance=D)
    assert poses.tobytes() == want.tobytes()
    assert len(graph.edges) == len(g.edges) == len(report["edges"])
    for a, b in zip(graph.edges, g.edges):
        assert a[:2] == b[:2] and a[4] == b[4] and a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    for e, row, l in zip(report["edges"], rows, line):
        assert (e["source"], e["target"], e["n"], e["rmse"], e["fitness"], e["l"]) == row + (float(l),)
    assert report["optimize"] == result
    # torch clouds on the device give the same bytes
    import torch
    dev = torch.device("cuda:0")
    p2, _, r2 = multiway.register_multiway([torch.from_numpy(c).to(dev) for c in clouds], poses0, max_distance=D, min_fitness=MIN_FITNESS)
    assert p2.tobytes() == poses.tobytes() and r2["edges"] == report["edges"]


def test_edge_rules_and_the_line_process(mods, scene, registered):
    clouds, truth, poses0 = scene
    poses, graph, report = registered
    N = len(clouds)
    edges = report["edges"]
    certain = [(e["source"], e["target"]) for e in edges if not e["uncertain"]]
    uncertain = [(e["source"], e["target"]) for e in edges if e["uncertain"]]
    assert certain == [(i + 1, i) for i in range(N - 1)]
    assert uncertain == [(N - 1, 0)], (uncertain, report["dropped"])                  # the ring's closure
    assert sorted((i, j) for (i, j, f) in report["dropped"]) == [(i, j) for i in range(N) for j in range(i + 2, N) if (i, j) != (0, N - 1)]
    for e in edges:
        print("edge %d -> %d: uncertain %d, n %d, rmse %.3g, fitness %.3f, l %.6f" % (e["source"], e["target"], e["uncertain"], e["n"],
                                                                                       e["rmse"], e["fitness"], e["l"]))
        assert e["l"] >= 0.25 and e["n"] >= 100 and (e["uncertain"] or e["l"] == 1.0)
        assert e["fitness"] >= (0.3 if not e["uncertain"] else MIN_FITNESS)
    opt = report["optimize"]
    print("pose graph:", opt)
    assert opt["n_pruned"] == 0 and opt["cost_end"] <= opt["cost_start"]
    assert poses[0].tobytes() == np.ascontiguousarray(poses0[0]).tobytes()
    # with a min_fitness no pair reaches, the graph is the chain of the certain edges
    icp, multiway, posegraph = mods
    p3, g3, r3 = multiway.register_multiway(clouds, poses0, max_distance=D, min_fitness=0.9)
    assert [e["uncertain"] for e in r3["edges"]] == [False] * (N - 1) and len(r3["dropped"]) == N * (N - 1) // 2 - (N - 1)
    assert r3["optimize"]["cost_start"] > 0 and r3["optimize"]["cost_end"] <= 1e-18 * r3["optimize"]["cost_start"]   # a tree: every edge is met
    # too few correspondences on a certain edge is an error
    with pytest.raises(icp.ICPError):
        multiway.register_multiway([clouds[0], clouds[0] + np.float32(10.0)], None, max_distance=D)       # ten units apart: no match


def test_optimised_poses_are_no_worse_than_the_chain(mods, scene, registered):
    """Pose errors against the generator, as the RMS displacement of each scan's own points, relative to scan 0: of the
    optimised poses, of the chain of the certain edges alone, and of each pairwise refine."""
    clouds, truth, poses0 = scene
    poses, graph, report = registered
    N = len(clouds)
    chain = [np.eye(4)]
    for i in range(1, N):
        T = [e[2] for e in graph.edges if (e[0], e[1]) == (i, i - 1)][0]
        chain.append(chain[i - 1] @ T)
    rel_true = [_inv(truth[0]) @ truth[i] for i in range(N)]
    e_opt = [PH.cloud_error(_inv(poses[0]) @ poses[i], rel_true[i], clouds[i]) for i in range(1, N)]
    e_chain = [PH.cloud_error(chain[i], rel_true[i], clouds[i]) for i in range(1, N)]
    e_start = [PH.cloud_error(_inv(poses0[0]) @ poses0[i], rel_true[i], clouds[i]) for i in range(1, N)]
    e_pair = [PH.cloud_error(e[2], _inv(truth[e[1]]) @ truth[e[0]], clouds[e[0]]) for e in graph.edges]
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))
    print("node errors, start     %s rms %.4g" % (["%.3g" % v for v in e_start], rms(e_start)))
    print("node errors, chain     %s rms %.4g" % (["%.3g" % v for v in e_chain], rms(e_chain)))
    print("node errors, optimised %s rms %.4g" % (["%.3g" % v for v in e_opt], rms(e_opt)))
    print("pairwise refine errors %s" % (["%d->%d %.3g" % (e[0], e[1], v) for e, v in zip(graph.edges, e_pair)],))
    assert rms(e_chain) < 0.2 * rms(e_start)                 # the registration itself worked
    assert rms(e_opt) <= rms(e_chain) + ACCURACY_MARGIN


def test_facade_returns_the_python_calls_poses_and_information_bytes(mods, scene, registered, tmp_path):
    """tests/multiway_app: RegisterMultiway (algorithms/multiway.h) on the scene's scans and start poses returns the poses,
    the edges and the line values of multiway.register_multiway, and ICPInformation (algorithms/icp_information.h) of scan 1
    against scan 0 returns ICP.information's matrix, count and rmse: every double read back from %.17g is the same double."""
    icp, multiway, posegraph = mods
    clouds, truth, poses0 = scene
    poses, graph, report = registered
    exe = apps.build_app(tmp_path, "multiway_app", apps.ICP_FACADE_LIBS)
    T = [e[2] for e in graph.edges if (e[0], e[1]) == (1, 0)][0]
    (tmp_path / "poses.txt").write_text("".join(" ".join("%.17g" % v for v in X.reshape(16)) + "\n" for X in list(poses0) + [T]))
    files = []
    for i, c in enumerate(clouds):
        files.append(str(tmp_path / ("scan%d.xyz" % i)))
        apps.write_xyz(files[-1], c)
    r = subprocess.run([exe, str(tmp_path / "poses.txt"), repr(D), repr(MIN_FITNESS)] + files, capture_output=True, text=True, timeout=apps.TIMEOUT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    got = np.array([[float(v) for v in ln.split()[2:18]] for ln in lines if ln.startswith("pose ")]).reshape(len(clouds), 4, 4)
    print("facade against python: max pose difference %.3g" % np.max(np.abs(got - poses)))
    assert got.tobytes() == poses.tobytes()
    edges = [ln.split() for ln in lines if ln.startswith("edge ")]
    assert len(edges) == len(report["edges"])
    for w, e in zip(edges, report["edges"]):
        assert (int(w[1]), int(w[2]), bool(int(w[3])), int(w[4]), float(w[5]), float(w[6]), float(w[7])) == \
               (e["source"], e["target"], e["uncertain"], e["n"], e["rmse"], e["fitness"], e["l"])
    g = [ln.split() for ln in lines if ln.startswith("graph ")][0]
    opt = report["optimize"]
    assert [int(g[2]), int(g[3])] == opt["iterations"] and int(g[5]) == opt["status_code"] and int(g[7]) == opt["n_pruned"]
    assert float(g[9]) == opt["cost_start"] and float(g[10]) == opt["cost_end"]
    w = [ln.split() for ln in lines if ln.startswith("info ")][0]
    info, n, rmse = icp.information(clouds[0], clouds[1], T, max_distance=D)
    assert int(w[1]) == n > 1000 and float(w[38]) == rmse
    assert np.array([float(v) for v in w[2:38]]).tobytes() == info.tobytes()


def test_command_line_writes_the_information_of_the_refined_pose(mods, tmp_path, s4p_lib_built):
    """The hippo fixture through `Super4PCS ... --icp 10 --icp-information f -m mat`: the file's pose is the matrix of -m, and
    its 6x6, count and rmse are ICP.information's for the two inputs at that pose; without --icp the flag is the usage exit."""
    icp, multiway, posegraph = mods
    from super4pcs_amd import build as B
    g = np.load(os.path.join(ROOT, "tests", "golden", "hippo_config1.npz"))
    Ps, Qu = g["Ps"].astype(np.float32), g["Qu"].astype(np.float32)
    delta, overlap, n_s = 0.01, 0.7, 200
    cli = B.build_cli()
    apps.write_obj(tmp_path / "P.obj", Ps); apps.write_obj(tmp_path / "Q.obj", Qu)
    f = tmp_path / "info.txt"
    mat, _ = apps.run_cli(cli, tmp_path / "P.obj", tmp_path / "Q.obj", delta, overlap, n_s, ["--icp", "10", "--icp-information", str(f)])
    lines = f.read_text().splitlines()
    assert lines[0] == "VERSION\t=\t1" and lines[1] == "POSE\t=" and lines[6] == "INFORMATION\t="
    T = np.array([[float(v) for v in ln.split()] for ln in lines[2:6]])
    got = np.array([[float(v) for v in ln.split()] for ln in lines[7:13]])
    n = int(lines[13].split("\t")[-1]); rmse = float(lines[14].split("\t")[-1])
    assert lines[13].startswith("CORRESPONDENCES\t=") and lines[14].startswith("RMSE\t=")
    assert np.array_equal(T, T.astype(np.float32).astype(np.float64)) and np.max(np.abs(T - mat)) <= 1e-6      # the float matrix of -m
    want, wn, wrmse = icp.information(Ps, Qu, T, max_distance=np.float32(4.0 * delta))
    print("hippo information: n %d (python %d), rmse %.6g, max |cli - python| / max %.3g" % (n, wn, rmse, np.max(np.abs(got - want)) / np.max(np.abs(want))))
    assert n == wn > 100 and rmse == wrmse
    assert got.tobytes() == want.tobytes()
    rc = subprocess.run([cli, "-i", str(tmp_path / "P.obj"), str(tmp_path / "Q.obj"), "-o", str(overlap), "-d", str(delta), "-t", "1000",
                         "-n", str(n_s), "--icp-information", str(f)], capture_output=True, text=True, timeout=60)
    assert rc.returncode == 1 and "Usage:" in rc.stderr
