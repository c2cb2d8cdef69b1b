"""CPU only: every constructed case of tests/matcher_edge_cases.py is in the regime it claims -- in the REFERENCE output alone.

For each case: the oracle's pair list equals the brute-force predicate (as test_pairs_match_reference_test_predicate), the
case's regime predicates hold on the oracle's lists, and the measured sizes are printed (they are DESIGN.md section 27's
table; run with -s to see them).  Where the reference's own sources are built (oracle/_ref), pairs and quads of the same
inputs are also compared with them.  tests/test_gpu_matcher_edges.py runs the same cases on the device.
"""
import numpy as np
import pytest

from tests import helpers as H
from tests import matcher_edge_cases as E

PAIR_CASES = E.pair_cases()


def _say(*a):
    print("[matcher-edge]", *a)


@pytest.fixture(scope="module")
def reflib_mod():
    reflib = pytest.importorskip("oracle.reflib")
    if not reflib.available():
        reflib.build()
    if not reflib.available():
        pytest.skip("oracle/_ref/libs4p_ref.so not built (needs the reference's sources)")
    return reflib


@pytest.fixture(scope="module")
def quad_refs(oracle_mod):
    out = {}
    for angle in (False, True):
        case = E.quad_cloud(angle)
        ref = E.prepare(oracle_mod, case)
        pairs = E.pairs_of(ref, case.calls[0])
        out[angle] = (case, ref, pairs, E.quad_lists(pairs))
    return out


@pytest.fixture(scope="module")
def disc_refs(oracle_mod):
    out = {}
    for which in ("sparse", "dense"):
        case = E.disc_case(which)
        ref = E.prepare(oracle_mod, case)
        out[which] = (case, ref, E.fused_reference(ref, case.base))
    return out


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pair_case_matches_brute_force_and_is_in_its_regime(oracle_mod, name):
    case = PAIR_CASES[name]
    ref = E.prepare(oracle_mod, case)
    first = None
    for k, call in enumerate(case.calls):
        pairs = E.pairs_of(ref, call)
        first = pairs if first is None else first
        brute = E.brute_pairs(case, ref, call)
        _say(name, "call", k, "n_Q", len(case.Q), "m", len(pairs), "undecided by the float64 restatement", len(brute[1]))
        assert E.matches_brute(pairs, brute)
        if k == 0:
            for rn, fn in case.regimes.items():
                holds, value = fn(pairs)
                _say(name, "regime", rn, "value", value)
                assert holds, (rn, value)
        if 0 < case.options.get("max_angle", -1.0) <= 90.0 and len(case.Q) > 2:      # (every call, so the figures of call 0 are printed too)
            s = set(map(tuple, pairs.tolist()))
            one = sum((b, a) not in s for a, b in s)
            sure, _ = E.brute_pairs(case._replace(options={}), ref, call)
            _say(name, "call", k, "ordered pairs kept", len(s), "of", len(sure), "without the filter; kept without their mirror", one,
                 "unordered pairs dropped whole", len(sure) // 2 - (len(s) + one) // 2)
            assert one > 0 and len(s) < len(sure)          # some ordered pairs kept, others of the same unordered pairs dropped
    assert len(first) > 0 or name == "pairs_n2_angle"      # (the two points' own pair is the base segment: its cosine rounds above 1)


def test_pair_attribute_case_exercises_every_filter(oracle_mod):
    """The attribute case must make each filter decide something: dropping it changes the list."""
    case = PAIR_CASES["pairs_attributes"]
    ref = E.prepare(oracle_mod, case)
    full = E.brute_pairs(case, ref, case.calls[0])[0]
    for drop in ("max_normal_difference", "max_color_distance"):
        opts = {k: v for k, v in case.options.items() if k != drop}
        fewer = E.brute_pairs(case._replace(options=opts), ref, case.calls[0])[0]
        _say("pairs_attributes without", drop, len(fewer), "with", len(full))
        assert len(fewer) > len(full)
    n, c = case.attrs
    zero, neg = (n * n).sum(1) == 0, c[:, 0] < 0
    p = np.asarray(full)
    assert zero[p].any(1).any() and neg[p].any(1).any()      # pairs that survive only because a filter is skipped for them
    assert case.calls[0][1] != 0.0 and len(case.Q) % 64 != 0


@pytest.mark.parametrize("angle", [False, True])
def test_quad_lists_are_in_their_regimes(quad_refs, angle):
    case, ref, pairs, lists = quad_refs[angle]
    m = ref["m"]
    dense, sparse = E.split_lists(pairs)
    _say(case.name, "n_Q", len(case.Q), "pairs", len(pairs), "between the clusters", len(dense))
    assert E.matches_brute(pairs, E.brute_pairs(case, ref, case.calls[0]))
    assert set(E.QUAD_M2) <= {len(p2) for _, p2, _ in lists.values()} and set(E.QUAD_M1) <= {len(p1) for p1, _, _ in lists.values()}
    for name, (p1, p2, regimes) in lists.items():
        quads = m.find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2)
        _say(case.name, name, "m1", len(p1), "m2", len(p2), "K", len(quads))
        for rn, fn in regimes.items():
            holds, value = fn(quads, p2)
            _say(case.name, name, "regime", rn, "value", value)
            assert holds, (name, rn, value)
    # the repeated lists really repeat, and the table size step lies between the two m1
    assert len(np.unique(lists["repeated_set2"][1], axis=0)) < len(lists["repeated_set2"][1])
    assert E.HASH_PER_PAIR * E.QUAD_M1[1] == E.HASH_MIN < E.HASH_PER_PAIR * E.QUAD_M1[2]


def test_a_base_inside_one_cluster_gives_no_quads(oracle_mod):
    """Why the quad cases use [A0, B0, A1, B1]: a base that lies inside one cluster finds nothing."""
    case = E.quad_cloud()._replace(base=(0, 1, 2, 3))
    ref = E.prepare(oracle_mod, case)
    pairs = E.pairs_of(ref, case.calls[0])
    dense, _ = E.split_lists(pairs)
    assert len(ref["m"].find_congruent(0.5, 0.5, E.QUAD_EPS, dense, dense[:256])) == 0


def test_disc_cloud_reaches_the_redo_and_the_fused_direct_append(disc_refs):
    (_, _, sp), (case, ref, de) = disc_refs["sparse"], disc_refs["dense"]
    for which, r in (("sparse", sp), ("dense", de)):
        _say("disc", which, "n_Q", len(case.Q), "m1", r["m1"], "m2", r["m2"], "K", r["K"], "C", r["C"], "best", r["best_count"], r["best_quad"])
    holds, value = E.redo(sp["m1"], de["m1"])
    _say("disc regime redo (m1 sparse, m1 dense)", value)
    assert holds
    holds, value = E.direct_append_fused(de["K"], de["m2"])
    _say("disc regime direct_append_fused K / tiles", value)
    assert holds
    assert 0 < de["C"] < de["K"] and de["found"] and sp["found"]          # the gate rejects some and passes some
    assert de["C"] <= 50000                                                # the CPU verifies every candidate: keep it modest


def test_gate_lists_mix_passing_and_failing_quads(disc_refs):
    case, ref, de = disc_refs["dense"]
    m = ref["m"]
    quads = m.find_congruent(de["inv"][0], de["inv"][1], 2.0 * case.delta, de["p1"], de["p2"])
    assert len(quads) == de["K"]
    for name, q in E.gate_lists(quads, len(case.Q)).items():
        nb, per, _, _ = m.try_congruent_set(np.asarray(case.base, np.int32), q)
        _say("gate", name, "K", len(q), "pass", nb, "fail", int((per < 0).sum()))
        if name.startswith("none"):
            assert nb == 0
        elif len(q) >= 63:
            assert 0 < nb < len(q)
        else:
            assert nb == len(q) == 1


def test_oracle_checksum_is_the_checksum_of_its_list(disc_refs):
    """The fused comparison on the device pins counts and checksums: the oracle's streaming checksum is tests.helpers.checksum of
    its own quad list, so an equal checksum pins the list and not only a number the two sides share."""
    case, ref, de = disc_refs["dense"]
    quads = ref["m"].find_congruent(de["inv"][0], de["inv"][1], 2.0 * case.delta, de["p1"], de["p2"])
    assert (len(quads), H.checksum(quads)) == (de["K"], de["quad_sum"])


def test_pairs_equal_the_reference_library(oracle_mod, reflib_mod):
    """The reference's own ExtractPairs on the constructed clouds (no base needed: the cases without max_angle and attributes)."""
    for name in ("pairs_n63", "pairs_n65", "pairs_n129", "pairs_n513", "pairs_dense", "pairs_small_radius"):
        case = PAIR_CASES[name]
        ref = E.prepare(oracle_mod, case)
        rm = reflib_mod.RefMatcher(oracle_mod.make_options(case.delta, 0.6, E.sample_size(case)))
        rm.init(case.Q, case.Q)
        assert np.array_equal(rm.cloud(1), ref["Qs"])
        for d, na, eps, b1, b2 in case.calls:
            want = rm.extract_pairs(float(E.F(d)), float(E.F(na)), float(E.F(eps)), b1, b2)
            assert np.array_equal(E.pairs_of(ref, (d, na, eps, b1, b2)), want), name


def test_quads_equal_the_reference_library(oracle_mod, reflib_mod):
    """FindCongruentQuadrilaterals needs the base's angle and the reference has no way to set a base: both sides SELECT (same
    RNG stream, as test_stages_match_reference_in_order), and the constructed lists go through both at those bases.  The
    lists between the clusters are all parallel to x and find nothing at a base whose segments are not, so the lists also run
    with a wide threshold (cells of a quarter of the cloud), where the filler pairs find quads at any angle."""
    case = E.quad_cloud()
    om = oracle_mod.Matcher(oracle_mod.make_options(case.delta, 0.6, E.sample_size(case)), full_counts=True)
    rm = reflib_mod.RefMatcher(oracle_mod.make_options(case.delta, 0.6, E.sample_size(case)))
    om.init(case.Q, case.Q); rm.init(case.Q, case.Q)
    d, na, eps, b1, b2 = case.calls[0]
    pairs = om.extract_pairs(d, na, eps, b1, b2)
    assert np.array_equal(pairs, rm.extract_pairs(d, na, eps, b1, b2))
    lists = E.quad_lists(pairs)
    bases = nonempty = 0
    for _ in range(12):
        r, o = rm.select_quadrilateral(), om.select_quadrilateral()
        assert r[0] == o[0]
        if not r[0]:
            continue
        assert np.array_equal(r[3], o[3]) and np.array_equal(r[4], o[4])
        bases += 1
        for thr in (E.QUAD_EPS, 0.2):
            for name, (p1, p2, _) in lists.items():
                want = rm.find_congruent(0.5, 0.5, thr, p1, p2)
                assert np.array_equal(om.find_congruent(0.5, 0.5, thr, p1, p2), want), (name, thr)
                nonempty += len(want) > 0
        if bases == 3:
            break
    _say("reference library: bases selected", bases, "non-empty quad lists compared", nonempty)
    assert bases > 0 and nonempty > 0          # a comparison of empty lists alone would say nothing
