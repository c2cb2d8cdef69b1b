"""The ICP edge-regime inputs (tests/icp_edge_cases.py) on the host: every case is in the regime it is meant for under the
restated grid plan and launch geometry, the CPU restatement, its brute force and numpy agree on it bit for bit, no case is
vacuous, and the crafted residual keys are exactly the wanted bits.  This is what makes tests/test_gpu_icp_edges.py
reviewable without a GPU."""
import math

import numpy as np
import pytest

from tests import icp_edge_cases as E
from tests import icp_helpers as H
from tests import icp_plane_helpers as PH
from tests import icp_robust_helpers as RH

F = np.float32


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    return H.build_cpu(tmp_path_factory.mktemp("icp_cpu"))


IDENTITY = np.eye(4)
# matched sources at the base pose, per case, pinned
MATCHED = {"one_target": 214, "identical_targets": 187, "flat": 3920, "needle": 8118, "enlarged": 37027, "box_faces": 9372,
           "far": 53992}


def _centred(case):
    c = E.frame(case.P)
    return c, (case.P - c).astype(F), (case.Q - c).astype(F)


@pytest.mark.parametrize("name", sorted(E.SMALL))
def test_restatements_agree_on_every_small_case(cpu, name):
    """icp_cpu_pass (grid), icp_cpu_brute and numpy_brute: the same idx and d2 bits, at the base pose and at a small motion."""
    case = E.SMALL[name]()
    c, Pc, Qc = _centred(case)
    for M in (IDENTITY, RH.motion(0.4, 0.003)):
        T = H.to_centred(E.pose(case, M), c).astype(F)
        ci, cd, cs = cpu.pass_(Pc, Qc, T, case.d)
        if len(Pc) * len(Qc) <= 4e9:
            bi, bd = cpu.brute(Pc, Qc, T, case.d)
            assert np.array_equal(ci, bi) and np.array_equal(cd, bd), name
        if len(Pc) * len(Qc) <= 4e7:
            ni, nd = H.numpy_brute(Pc, Qc, T, case.d)
            assert np.array_equal(ci, ni) and np.array_equal(cd, nd), name
        n = int(np.count_nonzero(ci >= 0))
        assert cs[0] == n and n >= 1, (name, n)
        if M is IDENTITY and name in MATCHED:
            assert n == MATCHED[name], (name, n)                 # a generator that drifts shows here
        if name in E.HAS_MISSES:
            assert n < len(Qc), name
        print("%s: n_P %d n_Q %d matched %d" % (name, len(Pc), len(Qc), n))


def test_every_case_is_in_its_regime():
    case = E.one_target()
    pl = E.plan(case.P, case.d)
    assert pl["cells"] == 1 and pl["enlargements"] == 0
    case = E.identical_targets()
    pl = E.plan(case.P, case.d)
    assert pl["cells"] == 1 and np.array_equal(pl["c"], case.P[0])
    case = E.flat()
    pl = E.plan(case.P, case.d)
    assert pl["dims"][2] == 1 and pl["dims"][0] > 100 and pl["enlargements"] == 0
    case = E.needle()
    pl = E.plan(case.P, case.d)
    assert pl["enlargements"] >= 2 and pl["dims"][0] >= 500 * pl["dims"][1] and pl["cells"] <= pl["cap"] / 1.2
    # not near a threshold: the unenlarged grid is far above the cap, and one enlargement fewer still overshoots it by a tenth
    ext = (case.P.max(0) - case.P.min(0)).astype(np.float64)
    assert np.prod(np.floor(ext / (1.02 * case.d)) + 1) >= 2 * pl["cap"]
    assert np.prod(np.floor(ext / (pl["h"] / 1.25)) + 1) >= 1.1 * pl["cap"]
    case = E.enlarged()
    pl = E.plan(case.P, case.d)
    assert pl["enlargements"] >= 2 and pl["h"] >= 2.0 * case.d and pl["cells"] <= pl["cap"] / 1.01
    ext = (case.P.max(0) - case.P.min(0)).astype(np.float64)
    assert np.prod(np.floor(ext / (1.02 * case.d)) + 1) >= 2 * pl["cap"]
    assert np.prod(np.floor(ext / (pl["h"] / 1.25)) + 1) >= 1.5 * pl["cap"]
    case = E.ragged(1)
    pl = E.plan(case.P, case.d)
    assert pl["enlargements"] == 0 and tuple(pl["dims"]) == (20, 20, 20)
    for n in E.RAGGED_N:
        assert len(E.ragged(n).Q) == n
    assert [E.launch(n) for n in (1, 63, 64, 65, 255, 256, 257)] == [(1, 0, 1)] * 5 + [(1, 1, 1), (2, 0, 1)]


def test_launch_geometry_of_the_large_cases():
    """2048 workgroups; every lane one trip at 524 288, the first lane two at 524 289, two to three at 1.3 M."""
    assert E.launch(E.FULL_LAUNCH_N[0]) == (2048, 1, 1)
    assert E.launch(E.FULL_LAUNCH_N[1]) == (2048, 1, 2)
    assert E.launch(600_000) == (2048, 1, 2)                  # full_launch's target
    assert E.launch(1_300_000) == (2048, 2, 3)
    assert 1_300_000 % (2048 * 256) % 256 != 0                # a ragged last trip


def test_far_case_sits_on_a_lattice_with_a_nonzero_frame(cpu):
    case = E.far()
    c, Pc, Qc = _centred(case)
    assert np.all(np.abs(c) > 1e3)
    assert len(np.unique(case.P[:, 0])) < 0.02 * len(case.P)           # a float step of 1e-3 at 1e4
    T = H.to_centred(case.T0, c).astype(F)
    ci, cd, _ = cpu.pass_(Pc, Qc, T, case.d)
    hit = ci >= 0
    assert 1000 < np.count_nonzero(hit) < len(Qc)
    # equal distances are common: many sources have their d2 shared with another source
    _, cnt = np.unique(cd[hit], return_counts=True)
    assert np.count_nonzero(cnt > 1) > 100


def test_box_faces_has_matched_queries_in_the_outer_cells_on_every_axis(cpu):
    case = E.box_faces()
    c, Pc, Qc = _centred(case)
    pl = E.plan(case.P, case.d, c)
    assert tuple(pl["dims"]) == (20, 20, 20) and pl["enlargements"] == 0
    ci, _, _ = cpu.pass_(Pc, Qc, np.eye(4, dtype=F), case.d)
    m = ci >= 0
    f = E.cell_coords(pl, Qc)
    for a in range(3):
        n = pl["dims"][a]
        counts = (np.count_nonzero(m & (f[:, a] == -1)), np.count_nonzero(m & (f[:, a] == n)),
                  np.count_nonzero(~m & ((f[:, a] == -1) | (f[:, a] == n))), np.count_nonzero((f[:, a] < -1) | (f[:, a] > n)))
        print("axis %d: matched in cell -1: %d, in cell n: %d, unmatched in those: %d, beyond: %d" % ((a,) + counts))
        assert min(counts) >= 50, (a, counts)
        assert not np.any(m & ((f[:, a] < -1) | (f[:, a] > n)))


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_key_pool_yields_the_wanted_bits(cpu, metric):
    """Every pool entry: numpy's key is the table's; through icp_cpu_pass the nearest target is the source's own lattice point
    and d2 carries the point key.  The formula of the point table holds wherever it is whole."""
    keys, off = E.key_pool(metric)
    assert np.all(np.diff(keys.astype(np.int64)) > 0) and len(keys) > 2000
    assert np.array_equal(E.key_bits(off, metric), keys)
    P = E.lattice()
    assert np.array_equal(E.frame(P), np.zeros(3, F))
    rng = np.random.default_rng(1)
    for _ in range(3):
        pick = rng.choice(len(keys), len(P), replace=False) if len(keys) >= len(P) else rng.integers(0, len(keys), len(P))
        Q = (P + off[pick]).astype(F)
        assert np.array_equal((Q - P).astype(F), off[pick])                  # the sum is exact
        ci, cd, _ = cpu.pass_(P, Q, np.eye(4, dtype=F), E.KEY_D)
        assert np.array_equal(ci, np.arange(len(P)))
        assert np.array_equal(cd.view(np.uint32), E.key_bits(off[pick], "point"))
        if metric == "plane":
            N = np.tile(np.array([0, 0, 1], F), (len(P), 1))
            _, info = RH.robust_sums(P, Q, np.eye(4, dtype=F), ci, cd, "plane", "trimmed", len(Q), E.KEY_D, Nc=N, trim_fraction=1.0)
            assert info[2] == int(keys[pick].max())
    if metric == "point":
        abc = np.rint(off.astype(np.float64) * 2.0 ** 14).astype(np.int64) - np.array([4096, 0, 0])
        s = (abc * abc).sum(1)
        whole = (s % 2 == 0) & (abc[:, 0] % 2 == 0)              # every operation exact
        assert np.array_equal(keys[whole].astype(np.int64), E.BASE + 4096 * abc[whole, 0] + s[whole] // 2)
        assert whole.sum() > 1000
        assert np.any((keys & 0xFF) == 0xFF) and np.any((keys & 0xFF00) == 0xFF00)


@pytest.mark.parametrize("metric", ["point", "plane"])
def test_crafted_multisets_are_what_they_claim(cpu, metric):
    """Per multiset: 1 <= k <= M < matches <= n_Q; the restatement's keys are the wanted ones; np.partition (RH.select) equals the
    literal digit walk; and the named property of the k-th key holds."""
    sets = E.crafted_multisets(metric)
    assert [m.name for m in sets] == ["upper24", "upper24_among_upper16", "bin_edge_shift16", "bin_edge_shift8", "bin_edge_shift0",
                                      "low_00", "low_ff", "second_ff", "duplicates"]
    for ms in sets:
        M, n_q = len(ms.keys), len(ms.Q)
        ci, cd, _ = cpu.pass_(ms.P, ms.Q, np.eye(4, dtype=F), E.KEY_D)
        n_match = int(np.count_nonzero(ci >= 0))
        assert n_match == n_q - E.N_FAR and M < n_q and np.array_equal(E.frame(ms.P), np.zeros(3, F))
        assert 1 <= M == n_match - (E.N_UNKEYED if metric == "plane" else 0)
        _, info = RH.robust_sums(ms.P, ms.Q, np.eye(4, dtype=F), ci, cd, metric, "trimmed", n_q, E.KEY_D, Nc=ms.N, trim_fraction=1.0)
        assert info[0] == M and info[2] == int(ms.keys.max())
        hit = ci >= 0
        keyed = hit & ms.N[np.where(hit, ci, 0)].any(1)
        got = E.key_bits((ms.Q[keyed] - ms.P[ci[keyed]]).astype(F), metric)
        assert np.array_equal(np.sort(got), np.sort(ms.keys))
        s = np.sort(ms.keys.astype(np.int64))
        for k in ms.ks:
            assert 1 <= k <= M
            assert math.ceil(E.trim_for(k, n_q) * n_q) == k
            thr, count = E.expected_selection(ms.keys, k)
            assert thr == int(RH.select(ms.keys.view(F), k).view(np.uint32)) == E.digit_walk(ms.keys, k) == s[k - 1]
            assert count == np.searchsorted(s, thr, side="right")
        km = (M + 1) // 2
        assert E.digit_walk(ms.keys, km) == s[km - 1]
        name, ks = ms.name, ms.ks
        if name.startswith("upper24"):
            lo = s[ks[0] - 1]
            assert all(s[k - 1] >> 8 == lo >> 8 for k in ks) and len({int(s[k - 1]) for k in ks}) == 3
            assert ks[2] - ks[0] + 1 == np.count_nonzero(s >> 8 == lo >> 8) >= 8
            if name == "upper24_among_upper16":
                assert np.all(s >> 16 == lo >> 16) and np.count_nonzero(s < lo) >= 100 and np.count_nonzero(s >> 8 > lo >> 8) >= 100
        elif name.startswith("bin_edge"):
            shift = int(name[len("bin_edge_shift"):])
            a, b = s[ks[0] - 1], s[ks[1] - 1]
            assert a >> (shift + 8) == b >> (shift + 8) and (a >> shift) + 1 <= b >> shift
        elif name == "low_00":
            assert s[ks[0] - 1] & 0xFF == 0
        elif name == "low_ff":
            assert s[ks[0] - 1] & 0xFF == 0xFF
        elif name == "second_ff":
            assert s[ks[0] - 1] & 0xFF00 == 0xFF00
        else:
            thr, count = E.expected_selection(ms.keys, ks[0])
            assert count == 1500 and np.count_nonzero(s == thr) == 1000 and np.count_nonzero(s < thr) < ks[0] < count


def test_trim_products():
    """ceil(trim_fraction * n_Q) on the double product: whole products stay, a rounding step above a whole number goes up."""
    up = 0
    for xi, n in E.TRIM_PRODUCTS:
        k = math.ceil(xi * n)
        exact = round(xi * n)
        assert k in (exact, exact + 1)
        up += k == exact + 1
        for metric in ("point", "plane"):
            ms = E.trim_product_case(n, metric)
            assert len(ms.Q) == n and 1 <= k <= len(ms.keys) < n
    assert math.ceil(0.1 * 30) == 3 and math.ceil(0.55 * 100) == 56 and math.ceil(0.5 * 30) == 15 and up >= 4


@pytest.mark.parametrize("name", ["far", "box_faces", "flat", "identical_targets", "needle", "one_target"])
def test_literal_normals_restatement_agrees_with_the_eigh_reference(tmp_path_factory, name):
    """tests/icp_plane_cpu/icp_normals_literal.cpp (k_normals term by term, the GPU module's bit-for-bit reference) against the
    independent restatement (brute-force neighbourhoods, numpy's eigh): the library's grid is plan()'s, zeros in the same
    places, |dot| >= 1 - 1e-6 where the two smallest eigenvalues are separated."""
    literal = PH.build_normals_literal(tmp_path_factory.mktemp("icp_normals_literal"))
    pcpu = PH.build_plane_cpu(tmp_path_factory.mktemp("icp_plane_cpu"))
    case = E.SMALL[name]()
    c, Pc, _ = _centred(case)
    G, dims, h = literal(Pc, case.d, case.d, 6)
    pl = E.plan(case.P, case.d, c)
    assert dims.tolist() == pl["dims"].tolist() and abs(h / pl["h"] - 1) < 1e-12
    k, c6 = pcpu.cov(Pc, case.d)
    N, w = PH.normals_from_cov(k, c6, 6)
    zero = ~N.any(1)
    assert np.array_equal(~G.any(1), zero)
    sep = (w[:, 1] >= 4 * w[:, 0]) & ~zero
    if name in ("far", "box_faces", "identical_targets"):
        assert sep.sum() > 0.1 * len(Pc)
    if sep.any():
        assert np.abs((G[sep].astype(np.float64) * N[sep].astype(np.float64)).sum(1)).min() >= 1 - 1e-6
    sub = np.arange(0, len(Pc), 7)
    assert np.array_equal(literal(Pc, case.d, case.d, 6, which=sub)[0], G[sub])
