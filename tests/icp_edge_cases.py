"""Inputs for the ICP edge-regime tests, in plain numpy, and a restatement of section 11's grid plan.

Every generator is deterministic (fixed seeds) and returns a Case: target P, source Q, max distance d and the base
transform T0 (caller frame) around which the tests move.  plan() and launch() say which regime an input is in; the
library exposes no grid accessor for ICP, so the tests assert the regime on these restatements.  The inputs sit well away
from the plan's thresholds, so plan() need not match the library's rounding.

crafted_multisets() builds sources whose residual keys are chosen bit for bit (the radix select's inputs): see there."""
import math
from collections import namedtuple

import numpy as np

F = np.float32
Case = namedtuple("Case", "name P Q d T0 origin", defaults=(np.zeros(3),))
K_BLOCK, K_MAX_BLOCKS = 256, 2048               # icp_src/s4p_icp_k_common.hip.hpp's launch geometry (blocks_for)
RAGGED_N = (1, 63, 64, 65, 255, 256, 257)
FULL_LAUNCH_N = (524_288, 524_289)              # 2048 x 256: the last single-trip size and the first two-trip one


def frame(P):
    """The float64 mean rounded to float: the library's frame up to one float step (its double sums differ in order)."""
    return np.asarray(P, F).astype(np.float64).mean(0).astype(F)


def plan(P, d, c=None):
    """DESIGN.md section 11's grid plan on P' = fl(P - c): h = 1.02 d (as float), times 1.25 until the dense grid has at
    most max(2^20, 2 n_P) cells; dims = floor((hi - lo) / h) + 1."""
    P = np.asarray(P, F)
    c = frame(P) if c is None else np.asarray(c, F)
    Pc = (P - c).astype(F)
    lo, hi = Pc.min(0).astype(np.float64), Pc.max(0).astype(np.float64)
    h = float(F(d)) * float(F(1.02))
    cap = max(1 << 20, 2 * len(P))
    k = 0
    while True:
        dims = (np.floor((hi - lo) / h) + 1).astype(np.int64)
        if int(np.prod(dims)) <= cap:
            break
        h *= 1.25
        k += 1
    return {"c": c, "lo": lo, "h": h, "dims": dims, "cells": int(np.prod(dims)), "enlargements": k, "cap": cap}


def cell_coords(pl, Xc):
    """floor((x - lo) / h) per axis (float64) of centred points under a plan()."""
    return np.floor((np.asarray(Xc, F).astype(np.float64) - pl["lo"]) / pl["h"])


def launch(n):
    """(workgroups, fewest trips of a lane, most trips of a lane) of a grid-stride launch over n items."""
    nb = max(1, min((n + K_BLOCK - 1) // K_BLOCK, K_MAX_BLOCKS))
    lanes = nb * K_BLOCK
    return nb, n // lanes, (n + lanes - 1) // lanes


def pose(case, M):
    """The caller-frame transform M T0 with the motion M taken about the case's origin (the clouds' own neighbourhood)."""
    S = np.eye(4); S[:3, 3] = case.origin
    Si = np.eye(4); Si[:3, 3] = -case.origin
    return S @ np.asarray(M, np.float64) @ Si @ case.T0


def _cube(seed=2, n=20_000):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (n, 3)).astype(F), rng


def one_target():
    rng = np.random.default_rng(101)
    return Case("one_target", np.zeros((1, 3), F), rng.normal(scale=0.05, size=(300, 3)).astype(F), 0.1, np.eye(4))


def identical_targets():
    rng = np.random.default_rng(102)
    return Case("identical_targets", np.zeros((1000, 3), F), rng.normal(scale=0.05, size=(257, 3)).astype(F), 0.1, np.eye(4))


def ragged(n):
    P, rng = _cube(2)
    Q = (P[:n] + rng.normal(scale=0.01, size=(n, 3))).astype(F)
    return Case("ragged_%d" % n, P, Q, 0.05, np.eye(4))


def flat():
    rng = np.random.default_rng(104)
    P = np.column_stack([rng.uniform(-1, 1, (20_000, 2)), np.zeros(20_000)]).astype(F)
    Q = (P[:4099] + rng.normal(scale=0.004, size=(4099, 3))).astype(F)
    return Case("flat", P, Q, 0.01, np.eye(4))


def needle():
    rng = np.random.default_rng(105)
    P = np.column_stack([rng.uniform(-500, 500, 30_000), rng.uniform(-0.5, 0.5, (30_000, 2))]).astype(F)
    Q = (P[:9001] + rng.normal(scale=0.02, size=(9001, 3))).astype(F)
    return Case("needle", P, Q, 0.05, np.eye(4))


def enlarged():
    rng = np.random.default_rng(106)
    P = rng.uniform(-0.5, 0.5, (50_000, 3)).astype(F)
    Q = (P + rng.normal(scale=0.002, size=P.shape)).astype(F)
    return Case("enlarged", P, Q, 0.004, np.eye(4))


def box_faces():
    """3 k sources inside the target's box, 6 k uniform in the box widened by 3 d, 6 k on a shell from d inside to 2.2 d
    outside the faces: queries in cell -1 and in cell n on every axis, matched and not, and queries beyond them."""
    P, rng = _cube(2)
    d = 0.05
    wide = rng.uniform(-0.5 - 3 * d, 0.5 + 3 * d, (6000, 3))
    s = rng.uniform(-1, 1, (6000, 3))
    shell = s / np.abs(s).max(1, keepdims=True) * (0.5 + rng.uniform(-d, 2.2 * d, (6000, 1)))
    return Case("box_faces", P, np.concatenate([P[:3000], wide, shell]).astype(F), d, np.eye(4))


FAR_SHIFT = np.array([1.0e4, -2.0e4, 3.0e3])


def far():
    """A bumpy pair moved to (1e4, -2e4, 3e3) and rounded to float: a float step of 1e-3 to 2e-3 there, so the surface sits
    on a lattice and equal distances are the rule.  T0 is the generator's pose carried to the shifted frame."""
    from super4pcs_amd import datasets as D
    P, Q, T = D.bumpy_pair(100_000, overlap=0.5, delta=0.004, seed=11)
    Pf = (P.astype(np.float64) + FAR_SHIFT).astype(F)
    Qf = (Q.astype(np.float64) + FAR_SHIFT).astype(F)
    T0 = np.array(T, np.float64)
    T0[:3, 3] = T[:3, 3] + FAR_SHIFT - T[:3, :3] @ FAR_SHIFT
    return Case("far", Pf, Qf, 4 * 0.004, T0, FAR_SHIFT)


def full_launch_pair():
    """The 600 k bumpy pair whose sources are cut to FULL_LAUNCH_N; its target takes two trips per lane on its own."""
    from super4pcs_amd import datasets as D
    P, Q, T = D.bumpy_pair(600_000, overlap=0.5, delta=0.004, seed=11)
    return Case("full_launch", P, Q, 4 * 0.004, np.array(T, np.float64))


def long_launch():
    from super4pcs_amd import datasets as D
    P, Q, T = D.bumpy_pair(1_300_000, overlap=0.5, delta=0.004, seed=11)
    return Case("long_launch", P, Q, 4 * 0.004, np.array(T, np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# dense variants and tiny targets: targets whose points have neighbours within d, so that the
# target-side walks (k_normals, k_color_gradient) sum something in the plan's other branch

DENSE_SEED = 77
CLUSTER = 10                                    # points per cluster centre
CLUSTER_HALF = 0.35                             # a cluster is uniform in +-0.35 d per axis: nearly every two of its points are within d


def _dense(parent, name, n_q, sigma, flatten=False):
    """The parent's first n_P / 10 points as cluster centres, 10 points per centre uniform in +-0.35 d per axis (z = 0
    afterwards for the flat case): the parent's n_P, d and grid regime, and about 10 points within d of every point (two
    points of a cluster are at most 0.7 d apart per axis; the host module asserts at least 6 neighbours everywhere).
    Q: the first n_q points plus noise, as the parent cuts its own."""
    case = parent()
    rng = np.random.default_rng(DENSE_SEED)
    m = len(case.P) // CLUSTER
    P = np.repeat(case.P[:m].astype(np.float64), CLUSTER, 0) + rng.uniform(-CLUSTER_HALF * case.d, CLUSTER_HALF * case.d, (m * CLUSTER, 3))
    if flatten:
        P[:, 2] = 0.0
    P = P.astype(F)
    Q = (P[:n_q] + rng.normal(scale=sigma, size=(n_q, 3))).astype(F)
    return Case(name, P, Q, case.d, np.eye(4))


def enlarged_dense():
    return _dense(enlarged, "enlarged_dense", 50_000, 0.002)


def needle_dense():
    return _dense(needle, "needle_dense", 9001, 0.02)


def flat_dense():
    return _dense(flat, "flat_dense", 4099, 0.004, flatten=True)


DENSE = {"enlarged_dense": enlarged_dense, "needle_dense": needle_dense, "flat_dense": flat_dense}


def dup_mixed():
    """5000 cube points and 50 of them 20 more times each, d = 0.1 (about 21 neighbours within d): duplicates inside ordinary
    neighbourhoods, for the sums whose terms are then exactly zero.  The copies follow the originals in the upload."""
    P, rng = _cube(3, 5000)
    pick = np.sort(rng.choice(5000, 50, replace=False))
    P = np.concatenate([P, np.repeat(P[pick], 20, 0)])
    Q = (P[:1500] + rng.normal(scale=0.02, size=(1500, 3))).astype(F)
    return Case("dup_mixed", P, Q, 0.1, np.eye(4))


TINY_N = (1, 5, 6, 63, 64, 65, 257)


def tiny_target(n):
    """The first n cube points scaled into a box of edge d / 2: every two within d, one cell; n = 5 is below min_neighbours = 6
    and n = 6 exactly at it."""
    d = 0.1
    P = (_cube(2)[0][:n].astype(np.float64) * (0.5 * d)).astype(F)
    rng = np.random.default_rng(300 + n)
    Q = (P[np.arange(40) % n] + rng.normal(scale=0.2 * d, size=(40, 3))).astype(F)
    return Case("tiny_target_%d" % n, P, Q, d, np.eye(4))


TINY = {"tiny_target_%d" % n: (lambda n=n: tiny_target(n)) for n in TINY_N}

TEXTURE_SCALE = {"needle": 0.02, "needle_dense": 0.02, "one_target": 4.0, "identical_targets": 4.0, "far": 4.0}


def texture_scale(name):
    """The scale at which icp_color_helpers.texture is sampled: about 1.5 periods across the cloud (the needle is 1000 long: a
    scale of 1 would alias along x), 10 periods per unit for the tiny targets (d / 2 across)."""
    if name.startswith("tiny_target"):
        return 10.0
    return TEXTURE_SCALE.get(name, 1.0)


def intensity(case, X=None):
    """texture() at coordinates relative to the case's origin (a field that varies over the cloud, wherever the cloud sits)."""
    from tests import icp_color_helpers as CH
    X = case.P if X is None else X
    return CH.texture(np.asarray(X, np.float64) - case.origin, texture_scale(case.name))


def caller_normals(P, seed):
    """Section 15's caller normals: random directions, not unit length, every 11th zero."""
    raw = np.random.default_rng(seed).normal(size=P.shape).astype(F) * 3
    raw[::11] = 0
    return raw


TILTED = np.array([0.36, -0.48, 0.8], F)          # a unit vector in double (0.1296 + 0.2304 + 0.64)


def gradient_normals(case):
    """The caller normals the gradient tests use per case, as (label, raw) pairs.  flat_dense: constant ones, (0, 0, 1) and a
    tilted unit vector with every 11th zero; random directions there put tangent planes edge-on to z = 0 and 17 points within a
    factor 2 of the gate, which is outside the restatement's input condition."""
    n = len(case.P)
    if case.name == "flat_dense":
        up = np.tile(np.array([0, 0, 1], F), (n, 1))
        tilted = np.tile(TILTED, (n, 1))
        tilted[::11] = 0
        return [("up", up), ("tilted", tilted)]
    return [("random", caller_normals(case.P, 4))]


def source_normals(n, seed):
    """Caller source normals as the generalized, coloured and rejection modules make them: not unit length, every 11th zero,
    one NaN."""
    raw = np.random.default_rng(seed).normal(size=(n, 3)).astype(F) * 3
    raw[::11] = 0
    if n > 5:
        raw[5, 0] = np.nan
    return raw


SUMS_MOTION = (0.3, 0.002)                      # degrees, shift: the one motion of the sums tests, about the case's origin
REJECTIONS = (dict(reciprocal=True), dict(reciprocal=True, normal_mode=1, normal_cos=float(np.cos(np.deg2rad(60.0)))))


def sums_inputs(case):
    """What the sums tests upload next to the clouds: raw target normals (the case's first gradient_normals), raw source normals,
    both intensities (one field: the source's is sampled where the base pose puts it) and the two poses."""
    from tests import icp_robust_helpers as RH
    Qm = case.Q.astype(np.float64) @ case.T0[:3, :3].T + case.T0[:3, 3]
    return dict(raw_p=gradient_normals(case)[0][1], raw_q=source_normals(len(case.Q), 8), Ip=intensity(case), Iq=intensity(case, Qm),
                poses=(pose(case, np.eye(4)), pose(case, RH.motion(*SUMS_MOTION))))


def cell_order_position(P, d):
    """Position of every point in the library's cell order under plan(): cells ascending (x fastest), upload order inside a cell."""
    pl = plan(P, d)
    Pc = (np.asarray(P, F) - pl["c"]).astype(F)
    f = np.clip(cell_coords(pl, Pc).astype(np.int64), 0, pl["dims"] - 1)
    key = (f[:, 2] * pl["dims"][1] + f[:, 1]) * pl["dims"][0] + f[:, 0]
    order = np.argsort(key, kind="stable")
    pos = np.empty(len(P), np.int64)
    pos[order] = np.arange(len(P))
    return pos


def gradient_sample(P, d, seed=9, n_random=3000, n_late=2000, margin=1000):
    """(sorted sample, positions under plan()'s cell order): n_random random points; n_late whose position is at least
    2048 x 256 + margin, so that a lane's second trip computes them even if the library's cell order moves a point by up to
    margin places against plan()'s (equal only up to the rounding of the plan); every point within margin places of
    position 2048 x 256, where the second trip begins (a stride that is off by one loses exactly that position); and the last
    margin / 2 positions, where it ends."""
    pos = cell_order_position(P, d)
    rng = np.random.default_rng(seed)
    lanes = K_MAX_BLOCKS * K_BLOCK
    late = np.flatnonzero(pos >= lanes + margin)
    seam = np.flatnonzero(((pos >= lanes - margin) & (pos < lanes + margin)) | (pos >= len(P) - margin // 2))
    pick = np.union1d(np.union1d(rng.choice(len(P), n_random, replace=False), rng.choice(late, n_late, replace=False)), seam)
    return pick, pos


SMALL = {"one_target": one_target, "identical_targets": identical_targets, "flat": flat, "needle": needle, "enlarged": enlarged,
         "box_faces": box_faces, "far": far}
SMALL.update({"ragged_%d" % n: (lambda n=n: ragged(n)) for n in RAGGED_N})
# cases that must leave some sources unmatched
HAS_MISSES = ("one_target", "identical_targets", "flat", "needle", "enlarged", "box_faces", "far")
# one entry per distinct target of SMALL (the ragged cases have box_faces' target and d: the gradients
# are a function of the target alone), the dense variants, dup_mixed and the tiny targets
GRADIENT_CASES = {k: v for k, v in SMALL.items() if not k.startswith("ragged_")}
GRADIENT_CASES.update(DENSE)
GRADIENT_CASES["dup_mixed"] = dup_mixed
GRADIENT_CASES.update(TINY)
SPARSE = ("one_target", "enlarged", "needle", "flat")       # section 15: almost no point has min_neighbours points within d
NO_GRADIENT = ("one_target", "identical_targets", "tiny_target_1", "tiny_target_5", "needle", "enlarged")
SUMS_CASES = HAS_MISSES + tuple(DENSE)


def gradient_floor(name, n):
    """The count of nonzero gradients a case must show (a predicate): none where no point has a system or every system is
    A = 0; more than half where the target is dense (a tenth of the caller normals are zero, and the cube's faces are thin);
    some for the flat cloud, where 481 of 20 000 points have 6 neighbours."""
    if name in NO_GRADIENT:
        return lambda k: k == 0
    if name == "flat":
        return lambda k: k > 0
    return lambda k: k > n / 2


def check_reject_counts(name, kw, pl, Qc, Tc, idx, why, counts):
    """What makes the degenerate cases bite under reciprocity, asserted on a rejection result (restated or the device's): one
    target keeps one pair at most, and exactly one when reciprocity is the only filter; of 1000 equal targets only index 0 is
    ever kept; box_faces keeps and rejects pairs whose moved source lies outside the target's box."""
    from tests import icp_robust_helpers as RH
    if name in ("one_target", "identical_targets"):
        assert counts[3] == 1 if not kw.get("normal_mode") else counts[3] <= 1, (name, kw, counts)
        assert counts[2] > 100 and np.all(idx[why == 0] == 0)
    if name == "box_faces":
        f = cell_coords(pl, RH.apply_f32(Tc, Qc))
        outside = np.any((f < 0) | (f >= pl["dims"]), axis=1)
        kept, rejected = np.count_nonzero(outside & (why == 0)), np.count_nonzero(outside & (why == 3))
        assert kept >= 10 and rejected >= 10, (kept, rejected)


# ---------------------------------------------------------------------------------------------------------------------
# crafted residual keys

KEY_D = 0.5
BASE = int(F(2.0 ** -4).view(np.uint32))        # bits of 2^-4: the point keys are BASE + t


def lattice():
    """The integer lattice [-32, 32]^2 x {0}: symmetric, so the frame is exactly zero and nothing is rounded by centring."""
    g = np.arange(-32, 33, dtype=F)
    X, Y = np.meshgrid(g, g)
    return np.column_stack([X.ravel(), Y.ravel(), np.zeros(X.size)]).astype(F)


def key_bits(off, metric):
    """The contract's key of a source P_j + off (identity transform, zero frame, normal (0, 0, 1)) in numpy: the float d2 in
    the contract's order, or float(r * r) with r in double."""
    off = np.asarray(off, F)
    if metric == "point":
        u = off[:, 0] * off[:, 0] + (off[:, 1] * off[:, 1] + off[:, 2] * off[:, 2])
    else:
        r = -off[:, 2].astype(np.float64)
        u = (r * r).astype(F)
    return np.ascontiguousarray(u, F).view(np.uint32)


def key_pool(metric):
    """(sorted distinct key bits, one offset per key) from a brute-force search.  point: dx = (4096 + a) 2^-14, dy = b 2^-14,
    dz = c 2^-14, so that d2 = 2^-4 (1 + (2^13 a + a^2 + b^2 + c^2) 2^-24) and the key is BASE + 4096 a + (a^2 + b^2 + c^2) / 2
    where a and that sum are even (every operation is then exact; otherwise the table records what float arithmetic gives).  plane: offsets
    along z only, dz = (2^23 + m) 2^-31, key float(dz^2)."""
    if metric == "point":
        a, b, c = np.meshgrid(np.arange(0, 41), np.arange(0, 80), np.arange(0, 80), indexing="ij")
        keep = (b <= c).ravel()
        abc = np.column_stack([a.ravel(), b.ravel(), c.ravel()])[keep]
        off = np.column_stack([(4096 + abc[:, 0]), abc[:, 1], abc[:, 2]]).astype(np.float64) * 2.0 ** -14
    else:
        m = np.arange(0, 1 << 17, dtype=np.float64)
        off = np.column_stack([np.zeros_like(m), np.zeros_like(m), (2.0 ** 23 + m) * 2.0 ** -31])
    off = off.astype(F)
    keys, first = np.unique(key_bits(off, metric), return_index=True)
    return keys, off[first]


Multiset = namedtuple("Multiset", "name metric P N Q keys ks")      # keys: the expected keys (uint32 bits); ks: ranks to select
N_FAR, N_UNKEYED = 25, 40


def _multiset(name, metric, pool, keys, ks, seed, n_far=N_FAR, n_unkeyed=N_UNKEYED):
    """Sources for the wanted keys (one lattice target each, in a shuffled order), N_FAR sources beyond d of everything and,
    for the plane metric, N_UNKEYED sources whose target has a zero normal: M = len(keys) < matches < n_Q."""
    pk, poff = pool
    P = lattice()
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, np.uint32)
    n_extra = n_far + (n_unkeyed if metric == "plane" else 0)
    assert len(keys) + n_extra <= len(P)
    tgt = rng.permutation(len(P))[:len(keys) + n_extra]
    pos = np.searchsorted(pk, keys)
    assert np.array_equal(pk[pos], keys)
    off = np.concatenate([poff[pos], np.tile(np.array([0.25, 0.25, 0.75], F), (n_far, 1)),
                          np.tile(np.array([0.0, 0.0, 0.125], F), (n_extra - n_far, 1))])
    N = np.tile(np.array([0, 0, 1], F), (len(P), 1))
    N[tgt[len(keys) + n_far:]] = 0
    order = rng.permutation(len(tgt))
    Q = (P[tgt] + off).astype(F)[order]
    return Multiset(name, metric, P, N, Q, keys, tuple(int(k) for k in ks))


def _bin_edge(keys, shift):
    """A rank k such that the k-th smallest key is the last of its bin of the digit at `shift` and the (k + 1)-th the first of
    the next bin, both within one bin of the digit above (so that this digit's pass decides): the middle such place."""
    s = np.sort(np.asarray(keys, np.uint32)).astype(np.int64)
    same_above = (s[1:] >> (shift + 8)) == (s[:-1] >> (shift + 8))
    edge = np.flatnonzero(same_above & ((s[1:] >> shift) != (s[:-1] >> shift))) + 1      # s[edge] opens a bin
    assert len(edge) > 0
    return int(edge[len(edge) // 2])


def crafted_multisets(metric):
    pool = key_pool(metric)
    U = pool[0].astype(np.int64)
    out = []
    seed = [200 if metric == "point" else 300]

    def add(name, keys, ks):
        seed[0] += 1
        out.append(_multiset(name, metric, pool, keys, ks, seed[0]))

    # keys equal in the upper 24 bits, distinct in the last byte: only the last pass decides
    top, cnt = np.unique(U >> 8, return_counts=True)
    g24 = None
    for t in top[np.argsort(-cnt, kind="stable")]:              # the fullest group with 100 keys on either side in its upper 16
        side = U[(U >> 16) == (t >> 8)] >> 8
        if np.count_nonzero(side < t) >= 100 and np.count_nonzero(side > t) >= 100:
            g24 = U[(U >> 8) == t]
            break
    assert g24 is not None and len(g24) >= 8
    add("upper24", g24, (1, (len(g24) + 1) // 2, len(g24)))
    # ... among keys that share the upper 16 bits only
    g16 = U[((U >> 16) == (g24[0] >> 16)) & ((U >> 8) != (g24[0] >> 8))]
    below, above = g16[g16 < g24[0]][-600:], g16[g16 > g24[-1]][:600]
    add("upper24_among_upper16", np.concatenate([below, g24, above]),
        (len(below) + 1, len(below) + (len(g24) + 1) // 2, len(below) + len(g24)))
    # the k-th key the last of its bin and the first of the next one, for each of the three lower digits
    rng = np.random.default_rng(7)
    for shift in (16, 8, 0):
        grp, cnt = np.unique(U >> (shift + 8), return_counts=True)
        # a group with several bins of this digit: the one with the most distinct digits, then the most keys
        best = max(grp, key=lambda v: (len(np.unique(U[(U >> (shift + 8)) == v] >> shift)), int(np.sum((U >> (shift + 8)) == v))))
        g = U[(U >> (shift + 8)) == best]
        if len(g) > 1300:
            g = np.sort(rng.choice(g, 1300, replace=False))
        keys = np.concatenate([g, g[::2]])                                    # every other key twice
        k = _bin_edge(keys, shift)
        add("bin_edge_shift%d" % shift, keys, (k, k + 1))
    # the k-th key with 0x00 / 0xFF in the lowest byte and with 0xFF in the second-lowest
    for name, mask, val in (("low_00", 0xFF, 0x00), ("low_ff", 0xFF, 0xFF), ("second_ff", 0xFF00, 0xFF00)):
        hit = np.flatnonzero((U & mask) == val)
        assert len(hit) > 0, name
        i = int(hit[len(hit) // 2])
        lo, hi = max(0, i - 300), min(len(U), i + 301)
        add(name, U[lo:hi], (i - lo + 1,))
    # heavy duplicates: one key 1000 times, straddling k
    i = len(U) // 2
    keys = np.concatenate([U[i - 500:i], np.full(1000, U[i]), U[i + 1:i + 501]])
    add("duplicates", keys, (900,))
    return out


def trim_for(k, n_q):
    """A trim fraction whose product with n_q is well inside (k - 1, k): ceil gives k whatever the rounding."""
    return (k - 0.5) / n_q


# (trim fraction, n_Q): products that are whole in double, and ones a rounding step above a whole number
# (0.1 * 30 is exactly 3.0 in double and stays 3; 0.55 * 100 = 55.00000000000001 goes to 56; 0.57 * 100 falls just below 57)
TRIM_PRODUCTS = ((0.5, 30), (0.25, 64), (0.75, 2000), (0.1, 30), (0.55, 100), (0.07, 100), (0.14, 50), (0.28, 25), (0.57, 100))


TRIM_N_FAR, TRIM_N_UNKEYED = 3, 2


def trim_product_case(n_q, metric="point"):
    """n_q sources with distinct keys (from the pool's middle) but TRIM_N_FAR far ones and, for the plane metric,
    TRIM_N_UNKEYED on zero normals: for the ceil(trim_fraction * n_Q) rule."""
    pool = key_pool(metric)
    i = len(pool[0]) // 2
    m = n_q - TRIM_N_FAR - (TRIM_N_UNKEYED if metric == "plane" else 0)
    return _multiset("trim_%d" % n_q, metric, pool, pool[0][i:i + m], (), 400 + n_q, n_far=TRIM_N_FAR, n_unkeyed=TRIM_N_UNKEYED)


def expected_selection(keys, k):
    """(k-th smallest key's bits, count of keys not above it)."""
    u = np.asarray(keys, np.uint32).view(F)
    thr = np.partition(u, k - 1)[k - 1]
    return int(thr.view(np.uint32)), int(np.count_nonzero(u <= thr))


def digit_walk(keys, k):
    """The library's four-pass walk restated literally: per 8-bit digit, most significant first, a histogram of the keys that
    agree with the prefix so far, then the bin that holds rank r."""
    u = np.asarray(keys, np.uint32).astype(np.int64)
    prefix, r = 0, int(k)
    for p in range(4):
        shift = 24 - 8 * p
        sel = u if p == 0 else u[(u >> (shift + 8)) == (prefix >> (shift + 8))]
        h = np.bincount((sel >> shift) & 0xFF, minlength=256)
        b = 0
        while b < 255 and r > h[b]:
            r -= int(h[b])
            b += 1
        prefix |= b << shift
    return prefix


def median_scale(thr_bits, d):
    """The contract's s = max(1.4826 sqrt(u_k), 1e-6 d)."""
    u = float(np.array([thr_bits], np.uint32).view(F)[0])
    return max(1.4826 * math.sqrt(u), 1e-6 * float(F(d)))
