"""-m gpu: k_pairs2, the set-1 preparation and k_quads at tile, stage, table and capacity edges.

The inputs are the constructed cases of tests/matcher_edge_cases.py; tests/test_matcher_edges_host.py shows on the CPU that
each is in the regime it claims.  Bar: every result is an integer or an index, so lists, order, counts and checksums equal
the CPU oracle's bit for bit (as tests/test_gpu_kernels.py); the pair lists also equal the brute-force predicate.
Environment knobs (S4P_PAIR_SPLIT, S4P_FUSE_PREP) are read by s4p_create: they are set before a context is constructed.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import matcher_edge_cases as E

pytestmark = pytest.mark.gpu

PAIR_CASES = E.pair_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PAIR_REFS = {}


def _context(case, ref, **limits):
    from super4pcs_amd import capi
    ctx = capi.Context(capi.make_options(case.delta, 0.6, E.sample_size(case), **case.options), **limits)
    ctx.set_clouds(ref["Ps"], ref["Qs"], ref["Qn"], ref["Qrgb"])
    if ref["has_attrs"]:
        ctx.set_base(ref["bx"], ref["bn"], ref["brgb"])
    else:
        ctx.set_base(ref["bx"])
    return ctx


def _limits(ctx):
    # capi.Context has no limits() of its own (only capi.Matcher has): s4p_get_limits is called on the context's handle through
    # the module's private _declare_matcher / _chk.  A public Context.limits() would be a source change; this file adds none.
    from super4pcs_amd import capi
    capi._declare_matcher(ctx.L)
    lim = capi.Limits()
    ctx._chk(ctx.L.s4p_get_limits(ctx.h, C.byref(lim)))
    return int(lim.max_pairs), int(lim.max_quads)


def _pair_ref(O, name):
    """The oracle's lists of a pair case, call by call on a fresh matcher, and the brute-force sets: computed once, never changed."""
    if name not in _PAIR_REFS:
        case = PAIR_CASES[name]
        ref = E.prepare(O, case)
        lists = [E.pairs_of(ref, call) for call in case.calls]
        brute = [E.brute_pairs(case, ref, call) for call in case.calls]
        for a in lists:
            a.setflags(write=False)
        _PAIR_REFS[name] = (case, ref, lists, brute)
    return _PAIR_REFS[name]


# ---------------------------------------------------------------------------------------------------------------------
# k_pairs2
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", E.PAIR_SPLITS)
@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_extract_pairs_equals_oracle_and_brute_force(oracle_mod, s4p_lib_built, monkeypatch, name, split):
    """Sizes 2 .. 513 (ragged last tile and chunk), the 256 + 256 clusters (a wave that appends on its own), exact duplicates
    and pair_distance < eps, the attribute filters: each for S4P_PAIR_SPLIT 1, 2, 4, plain and under max_angle (k_pairs2<true>;
    60 deg keeps at most one ordered pair of a candidate, the two `wide_angle` cases at 120 deg keep both of some).
    A context makes the calls of its case in the oracle's order (the octree's permutation persists on both sides)."""
    case, ref, lists, brute = _pair_ref(oracle_mod, name)
    monkeypatch.setenv("S4P_PAIR_SPLIT", str(split))
    ctx = _context(case, ref, max_pairs=1 << 18, max_quads=1 << 12)
    try:
        for call, want, bf in zip(case.calls, lists, brute):
            d, na, eps, b1, b2 = call
            got = ctx.extract_pairs(float(E.F(d)), float(E.F(na)), float(E.F(eps)), b1, b2)
            assert got.shape == want.shape
            assert np.array_equal(got, want)            # same pairs, same emission order
            assert E.matches_brute(got, bf)
    finally:
        ctx.close()
    assert sum(len(a) for a in lists) > 0 or name == "pairs_n2_angle"


def test_pair_capacity_exact_one_below_and_odd(oracle_mod, s4p_lib_built):
    """A pair capacity of exactly the count succeeds; one below, and an odd one, are refused with S4P_ERR_CAPACITY (the two
    ordered pairs of an entry fit together or not at all); a smaller list on the same context is right afterwards."""
    from super4pcs_amd import capi
    case = PAIR_CASES["pairs_n129"]
    big, small = (0.3, 0.0, 0.04, 0, 1), (0.3, 0.0, 0.01, 0, 1)
    ref = E.prepare(oracle_mod, case)
    want_big, want_small = E.pairs_of(ref, big), E.pairs_of(ref, small)
    m = len(want_big)
    assert m % 2 == 0 and 0 < len(want_small) < m - 3
    for cap in (m, m - 1, m - 3):
        ctx = _context(case, ref, max_pairs=cap, max_quads=64)
        try:
            assert _limits(ctx)[0] == cap
            if cap == m:
                assert np.array_equal(ctx.extract_pairs(*big), want_big)
            else:
                with pytest.raises(capi.S4PError) as ei:
                    ctx.extract_pairs(*big)
                assert ei.value.code == capi.S4P_ERR_CAPACITY
            assert np.array_equal(ctx.extract_pairs(*small), want_small)
        finally:
            ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# k_prep + k_quads, stage level
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["plain", "max_angle"])
def quad_setup(request, oracle_mod, s4p_lib_built):
    case = E.quad_cloud(request.param)
    ref = E.prepare(oracle_mod, case)
    pairs = E.pairs_of(ref, case.calls[0])
    lists = E.quad_lists(pairs)
    want = {n: ref["m"].find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2) for n, (p1, p2, _) in lists.items()}
    ctx = _context(case, ref, max_pairs=1 << 13, max_quads=1 << 18)
    yield dict(case=case, ref=ref, lists=lists, want=want, ctx=ctx)
    ctx.close()


QUAD_LIST_NAMES = ["m2_%d" % m for m in E.QUAD_M2] + ["m1_%d" % m for m in E.QUAD_M1] + ["repeated_set2", "tpp4", "tpp2", "tpp1",
                                                                                         "direct_append", "bisect", "sparse", "none"]


@pytest.mark.parametrize("name", QUAD_LIST_NAMES)
def test_find_congruent_equals_oracle(quad_setup, name):
    """m2 = 1 .. 513 (ragged tiles), m1 = 1 and both sides of the table's 4096 -> 8192 step, repeated entries, 4 / 2 / 1 threads
    per pair, the direct append past slot 512 of a tile and walks of hundreds of hops on a cell's four chains: same quads in
    the same order as the oracle, plain and with max_angle (k_quads<true>).  One context per setting takes every list."""
    p1, p2, _ = quad_setup["lists"][name]
    got = quad_setup["ctx"].find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2)
    assert got.shape == quad_setup["want"][name].shape
    assert np.array_equal(got, quad_setup["want"][name])


def test_every_constructed_quad_list_is_run(quad_setup):
    assert set(QUAD_LIST_NAMES) == set(quad_setup["lists"])


def test_one_context_over_time_dense_sparse_empty_dense(quad_setup):
    """The epoch-tagged hash is never cleared: lists that shrink and grow on one context, each call equal to the oracle's."""
    S = quad_setup
    ctx = _context(S["case"], S["ref"], max_pairs=1 << 13, max_quads=1 << 18)
    try:
        for name in ("direct_append", "sparse", "none", "empty", "m1_1", "direct_append", "m2_1", "tpp1"):
            if name == "empty":
                assert len(ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, np.zeros((0, 2), np.int32), S["lists"]["tpp1"][1])) == 0
                continue
            p1, p2, _ = S["lists"][name]
            assert np.array_equal(ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2), S["want"][name]), name
    finally:
        ctx.close()


def test_chunked_stage_call_full_list_loud_refusal_and_chunking_off(quad_setup):
    """s4p_find_congruent with max_quads far below K: ranges of the first pair set (none overflows here: the list is even, see
    the next test for the bisection), the full list in reference order; max_quads below the quads of one set-1 pair: the loud
    capacity error; chunking off: S4P_ERR_CAPACITY."""
    from super4pcs_amd import capi
    S = quad_setup
    p1, p2, _ = S["lists"]["tpp1"]
    want = S["want"]["tpp1"]
    K = len(want)
    key1 = {tuple(r): i for i, r in enumerate(p1.tolist())}
    per1 = np.bincount([key1[(a, b)] for a, b in want[:, :2].tolist()], minlength=len(p1))
    assert len(key1) == len(p1) and K > 16 * 1024 and per1.max() > 48
    assert E.chunk_ranges(len(p1), K, 48)[0] == 1          # ranges of one entry: the first that overflows cannot be split

    ctx = _context(S["case"], S["ref"], max_pairs=1 << 13, max_quads=1024)
    try:
        ctx.set_quad_chunking(True, 1024)
        assert _limits(ctx)[1] == 1024
        assert np.array_equal(ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2), want)
        ctx.set_quad_chunking(False)
        with pytest.raises(capi.S4PError) as ei:
            ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2)
        assert ei.value.code == capi.S4P_ERR_CAPACITY
        ctx.set_quad_chunking(True)
        p1s, p2s, _ = S["lists"]["m2_1"]
        assert np.array_equal(ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, p1s, p2s), S["want"]["m2_1"])      # and the context goes on
    finally:
        ctx.close()

    ctx = _context(S["case"], S["ref"], max_pairs=1 << 13, max_quads=48)
    try:
        ctx.set_quad_chunking(True, 48)
        with pytest.raises(capi.S4PError) as ei:
            ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2)
        assert ei.value.code == capi.S4P_ERR_CAPACITY and "one pair has more congruent quads" in str(ei.value)
    finally:
        ctx.close()


def test_chunked_stage_call_bisects_overflowing_ranges(quad_setup):
    """The `bisect` list at max_quads = CHUNK_CAP: first ranges that hold the adjacent heavy set-1 entries have more quads than the
    capacity while no single entry has, so they are halved and pushed back, and halves are halved again (the predicate, on the
    oracle's list, restates the library's range sizes).  The full list in reference order: halves pushed in the wrong order
    change the order, a dropped or overlapping half changes the count."""
    S = quad_setup
    p1, p2, regimes = S["lists"]["bisect"]
    want = S["want"]["bisect"]
    holds, value = regimes["chunk_bisection"](want, p2)
    assert holds, value
    assert len(want) > 4 * E.CHUNK_CAP
    ctx = _context(S["case"], S["ref"], max_pairs=1 << 13, max_quads=E.CHUNK_CAP)
    try:
        ctx.set_quad_chunking(True, E.CHUNK_CAP)
        assert _limits(ctx)[1] == E.CHUNK_CAP
        got = ctx.find_congruent(0.5, 0.5, E.QUAD_EPS, p1, p2)
        assert got.shape == want.shape
        assert np.array_equal(got, want)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the disc cloud: k_gate sizes and the fused pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disc(oracle_mod, s4p_lib_built):
    out = {}
    for which in ("sparse", "dense"):
        case = E.disc_case(which)
        ref = E.prepare(oracle_mod, case)
        out[which] = (case, ref, E.fused_reference(ref, case.base, threads=16))
    return out


DISC_LIMITS = dict(max_pairs=1 << 16, max_quads=1 << 15)


def test_try_congruent_set_gate_sizes(disc):
    """K = 1, 63, 64, 65, 257 with passing and failing quads mixed, and lists in which none passes: per-candidate values and
    the winner equal the oracle's."""
    case, ref, de = disc["dense"]
    m = ref["m"]
    base = np.asarray(case.base, np.int32)
    quads = m.find_congruent(de["inv"][0], de["inv"][1], 2.0 * case.delta, de["p1"], de["p2"])
    ctx = _context(case, ref, **DISC_LIMITS)
    try:
        for name, q in E.gate_lists(quads, len(case.Q)).items():
            nb, per, _, _ = m.try_congruent_set(base, q)
            r, got = ctx.try_congruent_set(base, q)
            assert np.array_equal(got, per), name
            assert r.n_verified == nb, name
            assert bool(r.has_best) == (nb > 0), name
            if nb:
                v = per[per >= 0]
                first = int(np.nonzero(per == v.max())[0][0])
                assert (r.best_count, r.best_rank, list(r.best_quad)) == (v.max(), first, q[first].tolist()), name
                ok, _, T = m.compute_rigid(base, q[first])
                assert ok and np.array_equal(np.array(r.best_transform, np.float32).reshape(4, 4), T), name
    finally:
        ctx.close()


def _check_fused(r, want, tag):
    assert (r.n_pairs1, r.n_pairs2) == (want["m1"], want["m2"]), tag
    assert (r.n_quads, r.quad_checksum) == (want["K"], want["quad_sum"]), tag
    assert (r.n_verified, r.cand_checksum) == (want["C"], want["cand_sum"]), tag
    assert bool(r.has_best) == want["found"], tag
    assert (r.best_count, list(r.best_quad)) == (want["best_count"], want["best_quad"]), tag


@pytest.mark.parametrize("fuse_prep", [None, "0"], ids=["default", "S4P_FUSE_PREP=0"])
def test_fused_pass_sparse_then_dense_base(disc, monkeypatch, fuse_prep):
    """try_base on the sparse base (its m1 sizes the next table under the 64 Ki floor), then on the dense one (m1 > 32 768: the
    fused preparation refuses entries, overflow bit 8, and the host redoes the base; K / tiles > 512: k_quads' direct append
    with its own gate and checksum adds), then the sparse one again: counts, checksums and the winner equal the oracle's,
    with the fused preparation and with S4P_FUSE_PREP=0."""
    if fuse_prep is not None:
        monkeypatch.setenv("S4P_FUSE_PREP", fuse_prep)
    case, ref, _ = disc["dense"]
    ctx = _context(case, ref, **DISC_LIMITS)
    try:
        for which in ("sparse", "dense", "sparse", "dense"):
            c, rf, want = disc[which]
            ctx.set_base(rf["bx"])
            r = ctx.try_base(np.asarray(c.base, np.int32), want["inv"][0], want["inv"][1])
            _check_fused(r, want, which)
    finally:
        ctx.close()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import oracle as O
from super4pcs_amd import capi
from tests import matcher_edge_cases as E
from tests.test_gpu_matcher_edges import _context, DISC_LIMITS
refs = [(c, E.prepare(O, c)) for c in (E.disc_case("sparse"), E.disc_case("dense"))]
ctx = _context(refs[1][0], refs[1][1], **DISC_LIMITS)
m1 = []
for c, rf in refs:
    ctx.set_base(rf["bx"])
    i1, i2 = E.invariants(rf["bx"])
    m1.append(int(ctx.try_base(np.asarray(c.base, np.int32), i1, i2).n_pairs1))
ctx.close()
print("M1", m1[0], m1[1])
"""


@pytest.mark.parametrize("fuse_prep", [None, "0"], ids=["default", "S4P_FUSE_PREP=0"])
def test_the_redo_really_runs(disc, fuse_prep):
    """The same two bases in a fresh process with S4P_TRACE_LAUNCH: the library's trace line at s4p_destroy counts the redo
    (prep_redos >= 1 with the fused preparation, 0 with S4P_FUSE_PREP=0)."""
    env = dict(os.environ, S4P_TRACE_LAUNCH="1")
    env.pop("S4P_FUSE_PREP", None)
    if fuse_prep is not None:
        env["S4P_FUSE_PREP"] = fuse_prep
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.split("M1")[1].split() == [str(disc["sparse"][2]["m1"]), str(disc["dense"][2]["m1"])]
    trace = [json.loads(l) for l in p.stderr.splitlines() if l.startswith('{"s4p_trace": "launch"')]
    assert len(trace) == 1 and trace[0]["bases"] >= 2
    if fuse_prep is None:
        assert trace[0]["prep_redos"] >= 1
    else:
        assert trace[0]["prep_redos"] == 0
