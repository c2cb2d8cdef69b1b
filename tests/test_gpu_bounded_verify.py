"""-m gpu: Verify under an early-exit bound (s4p_set_best_hint), candidate by candidate, against the oracle's full counts.

Every registration runs Verify with a bound: a candidate is abandoned once it can no longer EXCEED the best count so far.
Three pieces of device code carry that rule out -- k_sweep (the MFMA counting first pass over LDS query tiles), the lean
sweep of k_verify (wave_lcp_count_lean; queries in LDS or from global memory) and the tiled k_verify that scores k_sweep's
survivors tile by tile -- and a wrong bound there only shows in a registration when it happens to hit the winner.  Here each
base is scored at hints set right at the edges of its own counts (n = c - 1 and n = c for the largest counts c, both sides of
the tiled pass's per-tile switch at n = n_Q / 10), in every launch form of the bounded path, and the contract of
include/s4p_capi.h is checked per candidate (tests/bounded_helpers.py).  The last test builds clouds on which every query is an
inlier of every candidate, so that every upper bound the kernels form is tight: an off-by-one anywhere loses a candidate.
"""
import os

import numpy as np
import pytest

from tests import bounded_helpers as BH
from tests import helpers as H

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
MAX_QUADS = 3000                       # quads per base handed to try_congruent_set (a subsequence of the base's list, in order)

# sample size -> (delta, overlap, points of the synthetic pair); the spreads of test_the_sweep_pass_changes_no_result
CONFIGS = {400: (0.01, 0.6, 30000), 2000: (0.004, 0.8, 60000), 2700: (0.004, 0.8, 60000), 5000: (0.004, 0.8, 60000),
           20000: (0.004, 0.8, 60000)}

# what s4p_verify_kernel_info says for each launch form
LDS = "float queries in LDS"                         # lean k_verify<., true, true> (one sample in LDS)
TILES = "query tiles through LDS"                    # k_sweep + tiled k_verify<., true, true, true>
GLOBAL = "queries from global memory"                # lean k_verify<., false, true>

_CASES = {}


def _cases(O, n_s, n_bases=2):
    """(Ps, Qs, [(base, quads, per)]) of the first n_bases bases with verified candidates, oracle counts in full."""
    if n_s in _CASES:
        return _CASES[n_s]
    delta, overlap, n_pts = CONFIGS[n_s]
    P, Q, _ = H.small_pair(n_pts, delta=delta, seed=41, overlap=overlap)
    m = H.init_oracle(O, P, Q, delta, overlap, n_s)
    m.set_threads(THREADS)
    eps = 2.0 * delta
    out = []
    for _ in range(40):
        ok, i1, i2, base, bx = m.select_quadrilateral()
        if not ok:
            continue
        d1 = float(np.float32(np.linalg.norm(bx[0] - bx[1])))
        d2 = float(np.float32(np.linalg.norm(bx[2] - bx[3])))
        p1 = m.extract_pairs(d1, 0.0, eps, 0, 1)
        p2 = m.extract_pairs(d2, 0.0, eps, 2, 3)
        if len(p1) == 0 or len(p2) == 0:
            continue
        if n_s > 5000:                                     # (the full list runs to 10^9 quads: the congruent quads of a share of set 2)
            p1, p2 = p1[::8], p2[::512]
        quads = m.find_congruent(i1, i2, eps, p1, p2)
        if len(quads) == 0:
            continue
        quads = np.ascontiguousarray(quads[::max(1, len(quads) // MAX_QUADS)])
        nb, per, _bc, _bi = m.try_congruent_set(base, quads)
        if nb < 200:
            continue
        out.append((base.copy(), quads, per))
        if len(out) == n_bases:
            break
    assert len(out) == n_bases
    _CASES[n_s] = (m.cloud(0), m.cloud(1), out)
    return _CASES[n_s]


def _context(n_s, env, monkeypatch, Ps, Qs, **kw):
    from super4pcs_amd import capi
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    delta, overlap, _ = CONFIGS.get(n_s, (0.01, 0.6, 0))
    ctx = capi.Context(capi.make_options(delta, overlap, n_s, **kw.pop("opt", {})), **kw)
    ctx.set_clouds(Ps, Qs)
    ctx.profile_enable(True, False)
    for k in env:
        monkeypatch.delenv(k)
    return ctx


def _run(ctx, base, quads, n):
    ctx.set_best_hint(n)
    ctx.profile_get(reset=True)
    r, got = ctx.try_congruent_set(base, quads)
    return r, got, ctx.profile_get(reset=True)


def _edges(ctx, base, quads, per, n_q, swept, what):
    """The n = 0 run against the oracle, then every hint of BH.hint_list: assertions 1-6.  Returns {n: counts}."""
    r0, per0, _ = _run(ctx, base, quads, 0)
    BH.check_reference_run(r0, per0, per, quads)
    mx = int(per.max())
    out = {}
    for n in BH.hint_list(per, n_q):
        r, got, prof = _run(ctx, base, quads, n)
        BH.check_bounded(n, per, got, r, r0, what)
        if n == mx:
            assert prof.verify_pruned > 0, what + ": the bound never bit"
        if swept:
            assert prof.sweep_candidates > 0 and prof.sweep_survivors >= int((per > n).sum()), (what, n)
        else:
            assert prof.sweep_candidates == 0, (what, n)
        out[n] = got
    ctx.set_best_hint(0)
    return out


REGIMES = [
    # (sample, environment, launch form, k_sweep runs)
    (400, {}, LDS, False),
    (400, {"S4P_SWEEP_PASS": "1"}, LDS, True),
    (400, {"S4P_SWEEP_PASS": "1", "S4P_SWEEP_COARSE": "1"}, LDS, True),
    (2000, {}, LDS, False),
    (2000, {"S4P_SWEEP_PASS": "1"}, LDS, True),
    (2700, {}, TILES, True),
    (2700, {"S4P_SWEEP_COARSE": "1"}, TILES, True),
    (2700, {"S4P_VERIFY_TILED": "0"}, GLOBAL, True),
    (2700, {"S4P_SWEEP_PASS": "0"}, GLOBAL, False),
    (5000, {}, TILES, True),
    pytest.param(20000, {}, TILES, True, marks=pytest.mark.skipif(not os.environ.get("S4P_TEST_HEAVY"),
                                                                   reason="n_Q = 20 000 (bench extra): set S4P_TEST_HEAVY=1")),
]


@pytest.mark.parametrize("n_s,env,form,swept", REGIMES)
def test_bounded_counts_at_every_edge(oracle_mod, s4p_lib_built, monkeypatch, n_s, env, form, swept):
    """Per base and hint n: the gated-out pattern is the oracle's, every candidate above n keeps its exact count, every other
    one reports a lower bound, n_quads / n_verified / cand_checksum and (while the maximum exceeds n) the winner do not move,
    and the bound really abandons candidates.  2700 points: two tiles of 1536; 5000: three of 1792, the last one ragged."""
    Ps, Qs, cases = _cases(oracle_mod, n_s)
    n_q = Qs.shape[0]
    ctx = _context(n_s, env, monkeypatch, Ps, Qs)
    assert form in ctx.verify_kernel_info()
    if form == TILES:
        assert n_q > 2560 and (n_q <= 4096 if n_s == 2700 else n_q > 4096)
    for i, (base, quads, per) in enumerate(cases):
        _edges(ctx, base, quads, per, n_q, swept, "%d %s base %d" % (n_s, env, i))


GEOMETRIES = [{"S4P_VERIFY_THREADS": "256"}, {"S4P_VERIFY_THREADS": "448"}, {"S4P_VERIFY_THREADS": "1024"},
              {"S4P_VERIFY_BLOCKS": "64"}, {"S4P_VERIFY_BLOCKS": "4096"}, {"S4P_VERIFY_BLOCKS_SURV": "16"},
              {"S4P_SWEEP_COARSE": "1", "S4P_VERIFY_BLOCKS": "64"}]


def test_bounded_counts_do_not_depend_on_launch_geometry(oracle_mod, s4p_lib_built, monkeypatch):
    """Two tiles (k_sweep + tiled k_verify) at n = max - 1 and n = n_Q / 10 under other block sizes and grids, and with the
    coarse bitmap on 64 workgroups (many sweep rounds per workgroup: the survivor stage is flushed again and again): the
    per-candidate counts, abandoned lower bounds included, are those of the default geometry with the same bitmap (the
    bitmap decides which candidates k_sweep already drops, so it moves the lower bounds; the geometry must not)."""
    Ps, Qs, cases = _cases(oracle_mod, 2700)
    n_q = Qs.shape[0]
    hints = lambda per: sorted({int(per.max()) - 1, n_q // 10})
    ref = {}
    for bitmap in ({}, {"S4P_SWEEP_COARSE": "1"}):
        ctx = _context(2700, bitmap, monkeypatch, Ps, Qs)
        for i, (base, quads, per) in enumerate(cases):
            r0, _, _ = _run(ctx, base, quads, 0)
            for n in hints(per):
                r, got, _ = _run(ctx, base, quads, n)
                BH.check_bounded(n, per, got, r, r0, "default %s base %d" % (bitmap, i))
                ref[bool(bitmap), i, n] = (got, r0)
        ctx.close()
    for env in GEOMETRIES:
        ctx = _context(2700, env, monkeypatch, Ps, Qs)
        assert TILES in ctx.verify_kernel_info()
        for i, (base, quads, per) in enumerate(cases):
            for n in hints(per):
                want, r0 = ref["S4P_SWEEP_COARSE" in env, i, n]
                r, got, prof = _run(ctx, base, quads, n)
                BH.check_bounded(n, per, got, r, r0, "%s base %d" % (env, i))
                assert prof.sweep_candidates > 0
                assert np.array_equal(got, want), (env, i, n)
        ctx.close()


@pytest.mark.parametrize("force", [None, "1"])
def test_bounded_counts_with_the_angle_gate(oracle_mod, s4p_lib_built, monkeypatch, force):
    """max_angle with the device margin widened (S4P_ANGLE_TOL=0.02): many candidates whose Euler-angle gate the device leaves
    to the host.  They must reach the host whatever their count, so the gated-out pattern is the oracle's at every hint."""
    import ctypes as C
    O = oracle_mod
    delta, overlap, n_s, max_angle = 0.01, 0.6, 400, 30.0
    P, Q, _ = H.small_rotation_pair(30000, delta=delta)
    m = H.init_oracle(O, P, Q, delta, overlap, n_s, max_angle=max_angle)
    m.set_threads(THREADS)
    env = {"S4P_ANGLE_TOL": "0.02"}
    if force:
        env["S4P_SWEEP_PASS"] = force
    ctx = _context(n_s, env, monkeypatch, m.cloud(0), m.cloud(1), opt={"max_angle": max_angle})
    eps = 2.0 * delta
    tested = 0
    for _ in range(30):
        ok, i1, i2, base, bx = m.select_quadrilateral()
        if not ok:
            continue
        d1 = float(np.float32(np.linalg.norm(bx[0] - bx[1])))
        d2 = float(np.float32(np.linalg.norm(bx[2] - bx[3])))
        p1 = m.extract_pairs(d1, 0.0, eps, 0, 1)
        p2 = m.extract_pairs(d2, 0.0, eps, 2, 3)
        quads = m.find_congruent(i1, i2, eps, p1, p2) if len(p1) and len(p2) else np.zeros((0, 4), np.int32)
        if len(quads) == 0:
            continue
        nb, per, _bc, _bi = m.try_congruent_set(base, quads)
        if nb < 50:
            continue
        _edges(ctx, base, quads, per, m.cloud(1).shape[0], force is not None, "angle base %d" % tested)
        tested += 1
        if tested == 3:
            break
    assert tested == 3
    bs = (C.c_uint64 * 2)()
    ctx._chk(ctx.L.s4p_border_stats(ctx.h, bs))
    assert bs[0] > 0                                      # the host settled undecided candidates


def _trace(m, n_bases, delta):
    """The next n_bases bases of the oracle's sequence: (base, bx, i1, i2, quads, per) with full per-candidate counts."""
    eps = 2.0 * delta
    out = []
    while len(out) < n_bases:
        ok, i1, i2, base, bx = m.select_quadrilateral()
        if not ok:
            continue
        d1 = float(np.float32(np.linalg.norm(bx[0] - bx[1])))
        d2 = float(np.float32(np.linalg.norm(bx[2] - bx[3])))
        p1 = m.extract_pairs(d1, 0.0, eps, 0, 1)
        p2 = m.extract_pairs(d2, 0.0, eps, 2, 3)
        quads = m.find_congruent(i1, i2, eps, p1, p2) if len(p1) and len(p2) else np.zeros((0, 4), np.int32)
        per = m.try_congruent_set(base, quads)[1] if len(quads) else np.zeros(0, np.int32)
        out.append((base.copy(), bx.copy(), i1, i2, quads, per))
    return out


@pytest.mark.parametrize("n_s,env,form", [(400, {"S4P_SWEEP_PASS": "1"}, LDS), (2700, {}, TILES)])
def test_bounded_fused_pass_over_a_base_group(oracle_mod, s4p_lib_built, monkeypatch, n_s, env, form):
    """Three bases through s4p_try_base_async, then three s4p_try_base_wait, with S4P_LANES=3 and S4P_GROUP=3: one k_sweep /
    k_verify launch covers the group (the bases' candidates split by S.end over kGroupMax).  At a hint just below the smallest
    of the three maxima, and at n = n_Q / 10, every base's records obey the contract against the oracle's trace."""
    from super4pcs_amd import capi
    O = oracle_mod
    delta, overlap, n_pts = CONFIGS[n_s]
    P, Q, _ = H.small_pair(n_pts, delta=delta, seed=41, overlap=overlap)
    m = H.init_oracle(O, P, Q, delta, overlap, n_s)
    m.set_threads(THREADS)
    env = dict(env, S4P_LANES="3", S4P_GROUP="3")
    ctx = _context(n_s, env, monkeypatch, m.cloud(0), m.cloud(1))
    assert form in ctx.verify_kernel_info() and "groups of 3" in ctx.verify_kernel_info()
    BH.declare_async(ctx.L, capi.BaseResult)
    ctx.keep_candidate_records(True)
    n_q = m.cloud(1).shape[0]
    checked = 0
    for rnd in range(2):
        tr = _trace(m, 3, delta)
        maxima = [int(per.max()) for (_b, _x, _i1, _i2, _q, per) in tr if (per >= 0).any()]
        n = max(min(maxima) - 1 if rnd == 0 and maxima else n_q // 10, 1)
        ctx.set_best_hint(n)
        ctx.profile_get(reset=True)
        for (base, bx, i1, i2, _q, _p) in tr:
            ctx.set_base(bx)
            BH.try_base_async(ctx, base, i1, i2)
        for (base, bx, i1, i2, quads, per) in tr:
            r = BH.try_base_wait(ctx, capi.BaseResult)
            if len(quads) == 0:
                assert r.n_quads == 0
                continue
            gq, gc = ctx.last_candidates(len(quads))
            assert np.array_equal(gq, quads)
            want = _oracle_result(m, base, quads, per)
            BH.check_bounded(n, per, gc, r, want, "fused %d round %d" % (n_s, rnd), rank=False)
            vc, _vT = ctx.last_verified(max(want.n_verified, 1))
            BH.check_bounded(n, per[per >= 0], vc, None, None, "fused last_verified")
            checked += int(want.n_verified > 0)
        assert ctx.profile_get().verify_pruned > 0
    assert checked >= 4


def _oracle_result(m, base, quads, per):
    """What an s4p_base_result with no bound says, from the oracle: counts, checksum and the first maximum's quad and 4x4."""
    from types import SimpleNamespace
    v = per[per >= 0]
    r = SimpleNamespace(n_quads=len(quads), n_verified=len(v), cand_checksum=H.checksum(quads[per >= 0]),
                        best_count=int(v.max()) if len(v) else 0, best_quad=[0] * 4, best_transform=np.zeros(16, np.float32))
    if len(v):
        k = BH.first_max(per)
        ok, _rms, T = m.compute_rigid(base, quads[k])
        assert ok
        r.best_quad = quads[k].tolist()
        r.best_transform = T.reshape(16)
    return r


def test_bounded_counts_of_a_sliced_list(oracle_mod, s4p_lib_built, monkeypatch):
    """A quad list longer than the lane's buffers: s4p_try_congruent_set scores it in slices and folds the slices' winners.
    Under a bound the folded winner and every per-candidate count still obey the contract."""
    O = oracle_mod
    delta, overlap, n_s = 0.01, 0.6, 400
    P, Q, _ = H.small_pair(30000, delta=delta, seed=41, overlap=overlap)
    m = H.init_oracle(O, P, Q, delta, overlap, n_s)
    tr = [t for t in _trace(m, 4, delta) if len(t[4]) > 2500 and (t[5] >= 0).any()]
    assert tr
    for env in ({}, {"S4P_SWEEP_PASS": "1"}):
        ctx = _context(n_s, env, monkeypatch, m.cloud(0), m.cloud(1), max_quads=1000)
        for (base, _bx, _i1, _i2, quads, per) in tr:
            _edges(ctx, base, quads, per, n_s, bool(env), "sliced %s" % env)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# every query an inlier of every candidate: the kernels' upper bounds are all tight

K_TIGHT = 16


def _tight_clouds(n, cell_factor, delta=1.0):
    """Q: n points over a long box (x spans 0.0078 h * 65535, the quantised locate's worst case) holding a 4-point shape S at
    K_TIGHT places S + u_k; P: the base S + v and, for every k, Q + t_k - delta (1 - 1e-4) e_x with t_k = v - u_k.  Candidate k
    (quad S + u_k onto the base) is the translation t_k up to the fit's rounding, under which every query has a partner just
    inside delta along x.  The t_k are 5 apart in y (as in test_quantised_locate_cannot_lose_an_inlier_at_distance_delta) and
    step across the cell faces in x; S is large so that the fitted rotation's rounding stays far below the 1e-4 delta margin
    over the whole box."""
    rng = np.random.default_rng(5)
    h = (cell_factor or 1.002) * delta
    ext = 0.0078 * h * 65535.0
    S = 12.0 * np.array([[0.0, 0.0, 0.0], [1.7, 0.2, 0.1], [0.3, 1.9, 0.4], [1.1, 0.9, 2.3]])
    nb = n - 4 * K_TIGHT
    Qb = np.stack([rng.uniform(0, ext, nb), rng.uniform(0, 3, nb), rng.uniform(0, 3, nb)], axis=1)
    Qb[0, 0], Qb[1, 0] = 0.0, ext
    v = np.array([40.0, 0.5, 0.3])
    t = np.array([[0.0137 * k + 0.01, -5.0 * (k + 1), 0.0] for k in range(K_TIGHT)])
    Q = np.concatenate([S + (v - t[k]) for k in range(K_TIGHT)] + [Qb]).astype(np.float32)
    Ps = [S + v]
    for k in range(K_TIGHT):
        Pk = Q.astype(np.float64) + t[k]
        Pk[:, 0] -= delta * (1 - 1e-4)
        Ps.append(Pk)
    P = np.concatenate(Ps).astype(np.float32)
    return P, Q, np.arange(4, dtype=np.int32), np.arange(4 * K_TIGHT, dtype=np.int32).reshape(K_TIGHT, 4)


def _brute_counts(P, Q, Ts, delta):
    """float32 inlier counts with the Verify predicate ((T00 x + T01 y) + T02 z) + T03, |d|^2 <= delta^2 (P sorted by x, a
    window of +-delta around each query)."""
    F = np.float32
    o = np.argsort(P[:, 0], kind="stable")
    Px = P[o]
    out = []
    for T in Ts:
        tq = [((T[r, 0] * Q[:, 0] + T[r, 1] * Q[:, 1]) + T[r, 2] * Q[:, 2]) + T[r, 3] for r in range(3)]
        lo = np.searchsorted(Px[:, 0], tq[0] - F(1.01 * delta), "left")
        hi = np.searchsorted(Px[:, 0], tq[0] + F(1.01 * delta), "right")
        w = int((hi - lo).max())
        idx = np.minimum(lo[:, None] + np.arange(w)[None, :], len(Px) - 1)
        ok = np.arange(w)[None, :] < (hi - lo)[:, None]
        dx, dy, dz = tq[0][:, None] - Px[idx, 0], tq[1][:, None] - Px[idx, 1], tq[2][:, None] - Px[idx, 2]
        hit = ((dx * dx + (dy * dy + dz * dz)) <= F(delta) * F(delta)) & ok
        out.append(int(hit.any(axis=1).sum()))
    return np.array(out)


_TIGHT = {}


@pytest.mark.parametrize("cell_factor", [None, 1.6, 2.5])
@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("n,env,form", [(2000, {"S4P_SWEEP_PASS": "1"}, LDS), (5000, {}, TILES)])
def test_tight_bound_keeps_every_full_candidate(s4p_lib_built, monkeypatch, n, env, form, coarse, cell_factor):
    """Every candidate counts all n_Q queries (brute force on its own fitted transform, and the GPU without a bound), so at
    n = n_Q - 1 the k_sweep count, the per-tile L0 counts and confirmed + pending + unswept all equal n_Q exactly: each
    candidate must survive with count n_Q, and the first in reference order wins the tie whatever order the survivors came
    in.  2000 points: single-tile k_sweep + the lean LDS k_verify; 5000: three-tile k_sweep + tiled k_verify in its per-tile
    form (prune * 10 >= n_Q).  Own bitmap and S4P_SWEEP_COARSE=1; cells of 1.002 / 1.6 / 2.5 delta."""
    delta = 1.0
    P, Q, base, quads = _tight_clouds(n, cell_factor, delta)
    env = dict(env)
    if coarse:
        env["S4P_SWEEP_COARSE"] = "1"
    if cell_factor:
        env["S4P_CELL_FACTOR"] = str(cell_factor)
    from super4pcs_amd import capi
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx = capi.Context(capi.make_options(delta, 0.5, n), max_pairs=1 << 16, max_quads=1 << 16)
    ctx.set_clouds(P, Q)
    ctx.profile_enable(True, False)
    assert form in ctx.verify_kernel_info()
    ctx.keep_candidate_records(True)
    r0, per0 = ctx.try_congruent_set(base, quads)
    cnt, Ts = ctx.last_verified(K_TIGHT)
    assert len(cnt) == K_TIGHT and np.array_equal(cnt, per0)
    if (n, cell_factor) not in _TIGHT:
        _TIGHT[n, cell_factor] = _brute_counts(P, Q, Ts, delta)
    assert np.all(_TIGHT[n, cell_factor] == n)            # the construction: every query an inlier of every candidate
    assert np.all(per0 == n) and r0.best_count == n and r0.best_rank == 0
    ctx.set_best_hint(n - 1)
    ctx.profile_get(reset=True)
    r, got = ctx.try_congruent_set(base, quads)
    prof = ctx.profile_get(reset=True)
    assert prof.sweep_candidates == K_TIGHT and prof.sweep_survivors == K_TIGHT
    assert np.array_equal(got, per0), got
    assert (r.best_count, r.best_rank, r.n_verified) == (n, 0, K_TIGHT)
    assert list(r.best_quad) == list(r0.best_quad)
    # and at n = n_Q nothing can exceed the bound: every candidate is abandoned with a lower bound
    ctx.set_best_hint(n)
    r, got = ctx.try_congruent_set(base, quads)
    assert np.all((got >= 0) & (got <= n)) and r.best_count <= n and r.n_verified == K_TIGHT
    assert ctx.profile_get(reset=True).verify_pruned == K_TIGHT
