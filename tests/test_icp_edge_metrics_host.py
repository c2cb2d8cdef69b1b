"""The inputs of tests/test_gpu_icp_edge_metrics.py on the host: every new case of
tests/icp_edge_cases.py is in its regime under the restated grid plan; for every (case, normals, radius, min_neighbours) the
GPU module uses, the colour restatement's input condition holds (no eigenvalue ratio within a factor 2 of the gate) and the
floor on nonzero gradients is met, so that a comparison of zeros with zeros cannot pass for a test; which= rows of the
restatement are the full restatement's rows; and the generalized, coloured and rejection restatements run on the degenerate
cases and give the counts the GPU tests assert."""
import numpy as np
import pytest

from tests import icp_color_helpers as CH
from tests import icp_edge_cases as E
from tests import icp_gicp_helpers as GH
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_reject_helpers as JH

F = np.float32
MIN_NB = 6


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


@pytest.fixture(scope="module")
def literal(tmp_path_factory):
    return PH.build_normals_literal(tmp_path_factory.mktemp("icp_normals_literal"))


@pytest.fixture(scope="module")
def restated():
    """color_gradients at every target point, remembered per (case, normals): the far case costs 7 s."""
    memo = {}

    def get(case, label, Np, Pc):
        key = (case.name, label)
        if key not in memo:
            memo[key] = CH.color_gradients(Pc, Np, E.intensity(case), case.d, MIN_NB)
        return memo[key]

    return get


def _centred(case):
    c = E.frame(case.P)
    return c, (case.P - c).astype(F), (case.Q - c).astype(F)


def test_every_new_case_is_in_its_regime():
    for name, parent in (("enlarged_dense", E.enlarged), ("needle_dense", E.needle)):
        case, pl, pp = E.DENSE[name](), None, E.plan(parent().P, parent().d)
        pl = E.plan(case.P, case.d)
        assert len(case.P) == len(parent().P) and case.d == parent().d
        assert pl["enlargements"] == pp["enlargements"] == 4 and pl["h"] > 2.4 * case.d and pl["cells"] <= pl["cap"] / 1.01
        ext = (case.P.max(0) - case.P.min(0)).astype(np.float64)
        assert np.prod(np.floor(ext / (pl["h"] / 1.25)) + 1) >= 1.1 * pl["cap"]          # one enlargement fewer overshoots
        print(name, pl["dims"].tolist(), pl["h"] / case.d)
    assert E.plan(E.enlarged_dense().P, 0.004)["dims"].tolist() == [101, 101, 101]
    pl = E.plan(E.needle_dense().P, 0.05)
    assert pl["dims"][0] > 8000 and pl["dims"][1] == pl["dims"][2] == 9
    case = E.flat_dense()
    pl = E.plan(case.P, case.d)
    assert pl["dims"][2] == 1 and pl["dims"][0] > 100 and pl["enlargements"] == 0 and not case.P[:, 2].any() and len(case.P) == 20_000
    case = E.dup_mixed()
    assert len(case.P) == 6000 and len(np.unique(case.P, axis=0)) == 5000 and E.plan(case.P, case.d)["enlargements"] == 0
    for n in E.TINY_N:
        case = E.tiny_target(n)
        pl = E.plan(case.P, case.d)
        D = np.linalg.norm(case.P[:, None].astype(np.float64) - case.P[None].astype(np.float64), axis=2)
        assert len(case.P) == n and pl["cells"] == 1 and D.max() < 0.9 * case.d
    # the ragged cases bring no target of their own: the gradient tests visit box_faces' in their place
    box = E.box_faces()
    for n in E.RAGGED_N:
        case = E.ragged(n)
        assert case.P.tobytes() == box.P.tobytes() and case.d == box.d
    assert set(E.GRADIENT_CASES) | {"ragged_%d" % n for n in E.RAGGED_N} >= set(E.SMALL)


@pytest.mark.parametrize("name", sorted(E.GRADIENT_CASES))
def test_gradient_inputs_meet_the_restatements_condition_and_the_floors(literal, restated, name):
    """Caller normals of every case, and estimated ones (the literal restatement of k_normals) where section 15 does not list
    the case as SPARSE; r = d, min_neighbours = 6."""
    case = E.GRADIENT_CASES[name]()
    c, Pc, _ = _centred(case)
    setups = [(label, PH.normalise(raw)) for label, raw in E.gradient_normals(case)]
    if name not in E.SPARSE:
        setups.append(("estimated", literal(Pc, case.d, case.d, MIN_NB, threads=16)[0]))
    for label, Np in setups:
        g, ratio, k = restated(case, label, Np, Pc)
        near = (ratio >= 0.5e-6) & (ratio <= 2e-6)
        nonzero = int(g.any(1).sum())
        print("%s, %s normals: n %d, k >= %d at %d (mean %.1f), nonzero gradients %d, min ratio %s" % (
            name, label, len(Pc), MIN_NB, (k >= MIN_NB).sum(), k.mean(), nonzero, np.nanmin(ratio) if np.isfinite(ratio).any() else None))
        assert not near.any(), (name, label, np.flatnonzero(near)[:5])
        assert E.gradient_floor(name, len(Pc))(nonzero), (name, label, nonzero)
        if name in E.DENSE or name == "dup_mixed":
            assert (k >= MIN_NB).sum() >= 0.99 * len(Pc)
        if name in E.DENSE:
            assert np.all(k >= MIN_NB) and k.mean() >= 10.0


@pytest.mark.parametrize("name", ["far", "enlarged_dense"])
def test_which_rows_are_the_full_restatements_rows(restated, name):
    case = E.GRADIENT_CASES[name]()
    c, Pc, _ = _centred(case)
    label, raw = E.gradient_normals(case)[0]
    Np = PH.normalise(raw)
    g, ratio, k = restated(case, label, Np, Pc)
    which = np.sort(np.random.default_rng(5).choice(len(Pc), 2500, replace=False))
    gw, rw, kw = CH.color_gradients(Pc, Np, E.intensity(case), case.d, MIN_NB, which=which)
    assert gw.tobytes() == g[which].tobytes() and rw.tobytes() == ratio[which].tobytes() and np.array_equal(kw, k[which])
    assert gw.any(1).sum() > 1000
    kk, A, b = CH.gradient_systems(Pc, Np, E.intensity(case), case.d, which=which[:300])
    k2, A2, b2 = CH.gradient_systems(Pc, Np, E.intensity(case), case.d, which=which[:600])
    assert A.tobytes() == A2[:300].tobytes() and b.tobytes() == b2[:300].tobytes() and np.array_equal(kk, k2[:300])
    pairs = [np.concatenate(x) for x in zip(*CH.neighbour_pairs(Pc, case.d, which=which[:50]))]
    assert np.array_equal(np.unique(pairs[0]), which[:50]) and len(pairs[0]) == k[which[:50]].sum()


def test_second_trip_sample_of_the_full_launch_target(literal):
    """The 600 k target at r = d / 2: the points a lane computes on its second trip, under plan()'s cell order, and the sample
    the GPU module compares (input condition and floor on the restatement, with the literal restatement's normals)."""
    case = E.full_launch_pair()
    pick, pos = E.gradient_sample(case.P, case.d)
    assert np.array_equal(np.sort(pos), np.arange(len(case.P)))
    lanes = E.K_MAX_BLOCKS * E.K_BLOCK
    assert np.count_nonzero(pos >= lanes) == len(case.P) - lanes == 75_712
    assert np.all(np.diff(pick) > 0) and 7300 <= len(pick) <= 7500 and np.count_nonzero(pos[pick] >= lanes + 1000) >= 2000
    assert np.all(np.isin(np.arange(lanes - 1000, lanes + 1000), pos[pick])) and np.all(np.isin(np.arange(len(case.P) - 500, len(case.P)), pos[pick]))
    c, Pc, _ = _centred(case)
    Ne = np.zeros_like(Pc)
    Ne[pick] = literal(Pc, case.d, case.d, MIN_NB, which=pick, threads=16)[0]
    g, ratio, k = CH.color_gradients(Pc, Ne, E.intensity(case), case.d / 2, MIN_NB, which=pick)
    assert not np.any((ratio >= 0.5e-6) & (ratio <= 2e-6))
    late = pos[pick] >= lanes + 1000
    print("full_launch sample: %d points, %d late, nonzero %d (late %d), k mean %.1f" % (len(pick), late.sum(), g.any(1).sum(),
                                                                                     g[late].any(1).sum(), k.mean()))
    assert g.any(1).sum() > 0.5 * len(pick) and g[late].any(1).sum() > 0.5 * late.sum()


def _stored(case, cpu):
    c, Pc, Qc = _centred(case)
    inp = E.sums_inputs(case)
    Np, Nq = PH.normalise(inp["raw_p"]), PH.normalise(inp["raw_q"])
    G = CH.color_gradients(Pc, Np, inp["Ip"], case.d, MIN_NB)[0]
    return c, Pc, Qc, inp, Np, Nq, G


@pytest.mark.parametrize("name", ["one_target", "identical_targets", "box_faces"])
def test_restatements_run_on_the_degenerate_cases_and_give_the_counts(cpu, name):
    case = E.SMALL[name]()
    c, Pc, Qc, inp, Np, Nq, G = _stored(case, cpu)
    pl = E.plan(case.P, case.d, c)
    for T in inp["poses"]:
        Tc = H.to_centred(T, c).astype(F)
        fi, fd, _ = cpu.pass_(Pc, Qc, Tc, case.d)
        n = int(np.count_nonzero(fi >= 0))
        assert 0 < n < len(Qc)
        for eps in (1e-3, 1.0):
            s, sabs = GH.gicp_sums(Pc, Qc, Tc, fi, fd, Np, Nq, eps)
            assert np.all(np.isfinite(s)) and s[0] == s[2] == n
        for lam in (0.0, 0.968, 1.0):
            s, sabs = CH.color_sums(Pc, Qc, Tc, fi, fd, Np, G, inp["Ip"], inp["Iq"], lam)
            assert np.all(np.isfinite(s)) and s[0] == n and s[2] <= n
        for kw in E.REJECTIONS:
            ki, kd, why, cc = JH.restate(JH.cpu_search(cpu), Pc, Qc, Tc, case.d, Np=Np, Nq=Nq, forward=(fi, fd), **kw)
            print(name, kw, cc.tolist())
            assert cc[0] == n and cc[0] == cc[1] + cc[2] + cc[3]
            E.check_reject_counts(name, kw, pl, Qc, Tc, ki, why, cc)
