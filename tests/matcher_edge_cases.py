"""Constructed inputs for the pair / quad kernel edge tests, in plain numpy.

Every generator is deterministic and returns a Case: the clouds (P is always a copy of Q, so a base is four indices of the
same points), optional attributes, the options the oracle and the context share, the base, the stage arguments, and the
REGIME the case claims to reach as a predicate over the reference's own output (name -> function(ref) -> (holds, value)).
The predicates restate the kernels' constants (s4p_k_pairs.hip.hpp, s4p_k_quads.hip.hpp, s4p_capi_pass.inc) below; they
are conditions, not measurements: a case that stops meeting one fails the host test before any GPU sees it.

prepare() runs a case through the oracle (Matcher.init, so the oracle and the device see exactly the same points; every
case keeps n <= sample_size, which takes the cloud whole and in input order) and returns the reference output `ref`.
brute_pairs() is the reference's own test predicate (tests/pair_extraction.cc + testing.h) extended by the attribute and
segment-angle filters of PairCreationFunctor::process, as a float64 restatement.
"""
from collections import namedtuple

import numpy as np

F = np.float32

# the kernels' constants the predicates are written against
PAIR_TILE = 64            # k_pairs2: primitives per tile, slots per chunk
PAIR_STAGE = 256          # kPair2StageW: a wave appends on its own once n_st + 64 (ANGLE: + 128) exceeds it
PAIR_SPLITS = (1, 2, 4)   # S4P_PAIR_SPLIT
QUAD_TILE = 256           # kQuadThreads: set-2 pairs per tile of k_quads
QUAD_STAGE = 512          # kQuadStage: staged matches per tile; the rest is appended directly
TPP_4, TPP_2 = 64, 128    # pairs-with-a-chain per tile up to which a pair gets 4 / 2 threads for its cone mask
LONG_WALK = 64            # quads of one set-2 pair: all hang on the kSubChains = 4 chains of one cell
HASH_FLOOR = 65536        # prepare_base: floor of the fused preparation's table; an entry index above half of it is refused
HASH_MIN, HASH_PER_PAIR = 4096, 4      # hash_mask: slots = max(4 m1, 4096) rounded up to a power of two
PAIR_SIZES = (2, 63, 64, 65, 128, 129, 513)
QUAD_M2 = (1, 255, 256, 257, 513)
QUAD_M1 = (1, HASH_MIN // HASH_PER_PAIR, HASH_MIN // HASH_PER_PAIR + 1)      # 1, and both sides of the 4096 -> 8192 step
GATE_K = (1, 63, 64, 65, 257)
CHUNK_CAP = 256           # max_quads of the context that takes the `bisect` list: below a first range's quads, above one set-1 pair's

Case = namedtuple("Case", "name Q attrs delta options base calls regimes", defaults=(None, 0.01, {}, (0, 1, 2, 3), (), {}))
# attrs: None or (normals, colours) of Q (and of P = Q); options: keyword arguments of make_options beyond delta / overlap /
# sample_size; calls: tuples (pair_distance, pair_normals_angle, eps, bp1, bp2), made in this order; regimes speak of calls[0]


# ------------------------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------------------------
def _ball(rng, n, centre, radius):
    v = rng.normal(size=(n, 3))
    v *= (radius * rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    return v + np.asarray(centre, np.float64)


def two_clusters(n_a, n_b, n_fill=0, seed=1):
    """Clusters A (ids 0 .. n_a-1) and B (the next n_b) of radius 0.004, 0.5 apart along x, then uniform fillers: with
    pair_distance 0.5 and eps 0.02 every (A, B) combination is a pair, 2 n_a n_b ordered ones."""
    rng = np.random.default_rng(seed)
    parts = [_ball(rng, n_a, (0, 0, 0), 0.004), _ball(rng, n_b, (0.5, 0, 0), 0.004)]
    if n_fill:
        parts.append(rng.uniform((-0.25, -0.5, -0.5), (0.75, 0.5, 0.5), (n_fill, 3)))
    return np.concatenate(parts).astype(F)


def disc_cloud(rho, delta=0.01, n_small=3, n_fill=300, seed=2):
    """Two discs of radius rho perpendicular to the x axis at x = 0 and x = 0.5 (jittered grid of pitch 1.3 delta, two
    layers), two small discs of n_small points at (0.25, -/+0.2, 0) perpendicular to y for the second segment (it crosses
    the first at both midpoints: invariants 0.5, 0.5), and fillers.  Returns (cloud, dense base, sparse base): the dense
    base is [the points of A and B next to the axis, C0, D0]; the sparse one is a cross of four points of its own among the fillers."""
    rng = np.random.default_rng(seed)
    pitch = 1.3 * delta
    g = np.arange(-rho, rho + pitch, pitch)
    yy, zz = np.meshgrid(g, g, indexing="ij")
    yz = np.stack([yy.ravel(), zz.ravel()], 1)
    yz = yz[np.linalg.norm(yz, axis=1) <= rho]

    def disc(x0):
        lay = []
        for k in range(2):
            j = rng.uniform(-0.15, 0.15, (len(yz), 3)) * pitch
            lay.append(np.column_stack([np.full(len(yz), x0 + k * pitch), yz]) + j)
        return np.concatenate(lay)

    A, B = disc(0.0), disc(0.5)
    ang = np.linspace(0, 2 * np.pi, n_small, endpoint=False)
    small = np.stack([0.25 + 0.015 * np.cos(ang), np.zeros(n_small), 0.015 * np.sin(ang)], 1)
    C, D = small + (0, -0.2, 0), small + (0, 0.2, 0)
    fill = rng.uniform((-0.25, -0.5, -0.5), (0.75, 0.5, 0.5), (n_fill, 3))
    cross = np.array([(0.6, -0.3, 0.3), (0.6, -0.1, 0.3), (0.5, -0.2, 0.3), (0.7, -0.2, 0.3)])      # the sparse base: a cross of two 0.2 segments
    Q = np.concatenate([A, B, C, D, fill, cross]).astype(F)
    nA, nB = len(A), len(B)
    c0 = nA + nB
    s0 = len(Q) - 4
    near = lambda X, c: int(np.argmin(np.linalg.norm(X - np.asarray(c, np.float64), axis=1)))      # the disc's point next to its axis
    dense = (near(A, (0, 0, 0)), nA + near(B, (0.5, 0, 0)), c0, c0 + n_small)
    return Q, dense, (s0, s0 + 1, s0 + 2, s0 + 3)


# ------------------------------------------------------------------------------------------------------------------
# the oracle side
# ------------------------------------------------------------------------------------------------------------------
def sample_size(case):
    return max(len(case.Q), 16)


def prepare(O, case):
    """The oracle on the case: dict(m, Ps, Qs, Qn, Qrgb, bx, bn, brgb).  No point may be lost to the sampler."""
    m = O.Matcher(O.make_options(case.delta, 0.6, sample_size(case), **case.options), full_counts=True, use_kdtree=True)
    Q = np.ascontiguousarray(case.Q, F)
    if case.attrs is None:
        m.init(Q, Q)
        Ps, Qs, Qn, Qc = m.cloud(0), m.cloud(1), None, None
    else:
        n, c = case.attrs
        m.init(Q, Q, n, c, n, c)
        Ps, (Qs, Qn, Qc) = m.cloud(0), m.cloud(1, attrs=True)
    assert len(Ps) == len(Q) and len(Qs) == len(Q), "the sampler dropped points"
    cP, cQ, _, _ = m.frame()
    assert np.array_equal(Qs, (Q - cQ).astype(F)) and np.array_equal(Ps, (Q - cP).astype(F)), "the cloud is not in input order"
    m.set_base(np.asarray(case.base, np.int32))
    bx, bn, bc = m.get_base()
    return dict(m=m, Ps=Ps, Qs=Qs, Qn=Qn, Qrgb=Qc, bx=bx, bn=bn, brgb=bc, has_attrs=case.attrs is not None, delta=case.delta)


def brute_pairs(case, ref, call):
    """(sorted certain pairs, set of undecided pairs) of the reference's pair test predicate: |‖q_i - q_j‖ - d| <= eps (float
    distance, as tests/testing.h:172-194), then PairCreationFunctor::process's normal, colour and segment-angle filters in
    float64.  Undecided pairs exist under max_angle only (see below); without it the second set is empty."""
    d, nang, eps, bp1, bp2 = call
    Qs = ref["Qs"]
    diff = Qs[:, None, :] - Qs[None, :, :]
    dist = np.sqrt((diff[..., 0] * diff[..., 0] + (diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2])).astype(F))
    ok = ~(np.abs(dist.astype(np.float64) - np.float64(F(d))) > np.float64(F(eps)))
    n = len(Qs)
    ok &= np.arange(n)[:, None] > np.arange(n)[None, :]            # i = row (the primitive, q), j = column (p): i > j
    opt = case.options
    if opt.get("max_normal_difference", -1.0) > 0 and ref["has_attrs"]:
        N = ref["Qn"].astype(np.float64)
        nz = (N * N).sum(1) > 0
        a1 = np.linalg.norm(N[:, None] - N[None], axis=2)
        a2 = np.linalg.norm(N[:, None] + N[None], axis=2)
        fnd = np.minimum(np.abs(a1 - np.float64(F(nang))), np.abs(a2 - np.float64(F(nang))))
        thr = 0.5 * float(F(opt["max_normal_difference"])) * np.pi / 180.0
        ok &= ~((nz[:, None] & nz[None, :]) & (fnd > thr))
    if opt.get("max_color_distance", -1.0) > 0:
        mcd = float(F(opt["max_color_distance"]))
        Cc = ref["Qrgb"].astype(np.float64) if ref["has_attrs"] else np.full((n, 3), -1.0)
        b1, b2 = ref["brgb"][bp1].astype(np.float64), ref["brgb"][bp2].astype(np.float64)
        use = (Cc[None, :, 0] >= 0) & (Cc[:, None, 0] >= 0) & (b1[0] >= 0) & (b2[0] >= 0)
        good = (np.linalg.norm(Cc - b1, axis=1) < mcd)[None, :] & (np.linalg.norm(Cc - b2, axis=1) < mcd)[:, None]   # p = Q[j] ~ b1, q = Q[i] ~ b2
        ok &= ~(use & ~good)
    ii, jj = np.nonzero(ok)
    sure, maybe = [], []
    if opt.get("max_angle", -1.0) > 0:
        s1 = (ref["bx"][bp2] - ref["bx"][bp1]).astype(np.float64)
        s1 /= np.linalg.norm(s1)
        s2 = (Qs[ii] - Qs[jj]).astype(np.float64)
        s2 /= np.linalg.norm(s2, axis=1)[:, None]
        dd = np.clip(s2 @ s1, -1.0, 1.0)
        lim = float(F(opt["max_angle"])) * np.pi / 180.0
        # the reference forms the cosine in float: within 1e-5 of the threshold, or of +-1 (acosf of a cosine that rounded above 1 is
        # NaN: no pair), this float64 restatement does not decide
        open_ = (np.abs(np.abs(dd) - 1.0) < 1e-5)
        for sign, swap in ((1.0, False), (-1.0, True)):
            a = np.arccos(sign * dd)
            for i, j, k, u in zip(ii.tolist(), jj.tolist(), (a <= lim).tolist(), (open_ | (np.abs(a - lim) < 1e-5)).tolist()):
                if u:
                    maybe.append((i, j) if swap else (j, i))
                elif k:
                    sure.append((i, j) if swap else (j, i))
    else:
        for i, j in zip(ii.tolist(), jj.tolist()):
            sure.append((j, i)); sure.append((i, j))
    return sorted(sure), set(maybe)


def matches_brute(pairs, brute):
    """The oracle's list against brute_pairs(): every certain pair, nothing but certain and undecided ones, no repetition."""
    sure, maybe = brute
    got = sorted(map(tuple, np.asarray(pairs).reshape(-1, 2).tolist()))
    return len(set(got)) == len(got) and sorted(set(got) - maybe) == sure


def pairs_of(ref, call):
    """The oracle's ordered pair list of one call (the calls of a case must be made in order: the octree's permutation persists)."""
    d, nang, eps, bp1, bp2 = call
    return ref["m"].extract_pairs(float(F(d)), float(F(nang)), float(F(eps)), bp1, bp2)


# ------------------------------------------------------------------------------------------------------------------
# regime predicates over the reference's output
# ------------------------------------------------------------------------------------------------------------------
def wave_own_append(pairs, n_q, angle=False, split=4):
    """k_pairs2's wave-own append.  E_t = accepted (pId > j) tests -- under ANGLE: emitted ordered pairs -- whose primitive
    lies in tile t.  They are spread over n_chunks * split items of that tile, so one item holds at least E_t / (n_chunks
    split): more than the whole stage (256) means the wave flushes on its own whatever the earlier items left.  n_seq <= n_Q
    (PairOctree::build drops cells no sphere touches, flatten() emits the rest once), so ceil(n_Q / 64) bounds n_chunks from
    above and the value from below."""
    p = np.asarray(pairs).reshape(-1, 2)
    if len(p) == 0:
        return False, 0.0
    prim = p.max(1) // PAIR_TILE
    e = np.bincount(prim) if angle else np.bincount(prim[p[:, 0] < p[:, 1]])
    n_chunks = (n_q + PAIR_TILE - 1) // PAIR_TILE
    v = float(e.max()) / (n_chunks * split)
    return v > PAIR_STAGE, v


def per_pair2_counts(quads, p2):
    """Quads per set-2 list position.  A quad is found by its two set-2 ids; lists with repeated entries are counted per
    distinct entry (each repetition finds the same quads)."""
    p2 = np.asarray(p2).reshape(-1, 2)
    key2 = p2[:, 0].astype(np.int64) << 32 | p2[:, 1].astype(np.int64)
    cnt = np.zeros(len(p2), np.int64)
    if len(quads):
        q = np.asarray(quads)
        kq = q[:, 2].astype(np.int64) << 32 | q[:, 3].astype(np.int64)
        u, c = np.unique(kq, return_counts=True)
        mult = {k: int(np.sum(key2 == k)) for k in u.tolist()}
        look = dict(zip(u.tolist(), c.tolist()))
        cnt = np.array([look.get(k, 0) // max(mult.get(k, 1), 1) for k in key2.tolist()], np.int64)
    return cnt


def direct_append_stage(quads, p2):
    """k_quads' direct append, stage call (tiles are 256 consecutive entries of the caller's list): most matches in a tile > 512."""
    c = per_pair2_counts(quads, p2)
    v = max(int(c[i:i + QUAD_TILE].sum()) for i in range(0, len(c), QUAD_TILE))
    return v > QUAD_STAGE, v


def direct_append_fused(K, m2):
    """... fused path (device order): the mean over the tiles exceeds the stage, so some tile does."""
    v = K / max((m2 + QUAD_TILE - 1) // QUAD_TILE, 1)
    return v > QUAD_STAGE, v


def long_walk(quads, p2):
    v = int(per_pair2_counts(quads, p2).max())
    return v >= LONG_WALK, v


def threads_per_pair(quads, p2, want):
    """The tile's pairs with a chain decide 4 / 2 / 1 threads per pair.  A set-2 pair with a quad has a chain, and no more
    pairs than the tile holds can have one: a list of <= 64 pairs gets 4; 65 .. 128 pairs of which >= 65 have a quad get 2;
    a full tile in which >= 129 pairs have a quad gets 1."""
    c = per_pair2_counts(quads, p2)
    m2, first = len(c), int((c[:QUAD_TILE] > 0).sum())
    if want == 4:
        return m2 <= TPP_4 and first > 0, (m2, first)
    if want == 2:
        return TPP_4 < m2 <= TPP_2 and first > TPP_4, (m2, first)
    return m2 >= QUAD_TILE and first > TPP_2, (m2, first)


def chunk_ranges(m1, K, cap):
    """The ranges of the first pair set s4p_find_congruent enumerates again once K quads overflowed a capacity of cap, computed
    as the library computes them (s4p_capi_abi_stages.inc): target = cap 6/10, nch = ceil(K / target), step = ceil(m1 / nch)."""
    target = max(cap * 6 // 10, 1)
    nch = (K + target - 1) // target
    step = max(1, (m1 + nch - 1) // nch)
    return step, [(a, min(a + step, m1)) for a in range(0, m1, step)]


def chunk_bisection(quads, p1, cap):
    """The chunked stage call's bisection.  A range overflows when it holds more than cap quads; it is then halved at
    mid = lo + (hi - lo) / 2 and both halves are pushed back, the lower one on top.  Required: some first range of `step`
    consecutive set-1 entries holds more than cap quads while no single entry does (else the call ends in the loud refusal),
    and some half overflows again (depth >= 2: a re-pushed half is itself split while its sibling and the later first ranges
    wait below it, so the order of the pushes decides the order of the list).  Value: (step, ranges, ranges that overflow,
    most quads in a range, most quads of one entry, depth)."""
    p1 = np.asarray(p1).reshape(-1, 2)
    key1 = {tuple(r): i for i, r in enumerate(p1.tolist())}
    assert len(key1) == len(p1), "a quad is attributed to its set-1 entry by value: the list must not repeat"
    q = np.asarray(quads).reshape(-1, 4)
    per1 = np.bincount([key1[(a, b)] for a, b in q[:, :2].tolist()], minlength=len(p1))
    cs = np.concatenate([[0], np.cumsum(per1)])
    step, rg = chunk_ranges(len(p1), len(q), cap)

    def depth(a, b):
        if cs[b] - cs[a] <= cap:
            return 0
        mid = a + (b - a) // 2
        return 1 + max(depth(a, mid), depth(mid, b))

    sums = [int(cs[b] - cs[a]) for a, b in rg]
    over = sum(x > cap for x in sums)
    dep = max(depth(a, b) for a, b in rg)
    return over > 0 and int(per1.max()) <= cap and dep >= 2, (step, len(rg), over, max(sums), int(per1.max()), dep)


def both_orders(pairs):
    """ANGLE with max_angle > 90 deg: cos_min < 0, so a candidate whose cosine lies in [cos_min, -cos_min] emits (j,i) AND (i,j) in
    one batch (emit_a and emit_b of the same lane: the `+ 128` threshold, the st_f = 0 / 1 interleave).  Value: unordered pairs
    present in both orders."""
    s = set(map(tuple, np.asarray(pairs).reshape(-1, 2).tolist()))
    v = sum((b, a) in s for a, b in s) // 2
    return v > 0, v


def one_sided(pairs):
    """... and ordered pairs kept without their mirror (only one of emit_a / emit_b)."""
    s = set(map(tuple, np.asarray(pairs).reshape(-1, 2).tolist()))
    v = sum((b, a) not in s for a, b in s)
    return v > 0, v


def redo(m1_sparse, m1_dense):
    """The fused preparation's overflow bit 8: the table of the dense base is sized from the sparse one (6 m1 slots, under the
    64 Ki floor), and an entry index above half of the floor's slots is refused."""
    return HASH_PER_PAIR * (m1_sparse * 3 // 2) < HASH_FLOOR and m1_dense > HASH_FLOOR // 2, (m1_sparse, m1_dense)


# ------------------------------------------------------------------------------------------------------------------
# pair cases
# ------------------------------------------------------------------------------------------------------------------
ANGLE_OPTS = {"max_angle": 60.0}      # keeps (j,i) or (i,j) of most unordered pairs and neither of those within 30 deg of the normal plane
# cos_min = -0.5: a pair within 30 deg of the normal plane of the base segment is kept in BOTH orders (60 deg cannot: dd >= 0.5 and
# -dd >= 0.5 exclude each other), the others in one
WIDE_ANGLE_OPTS = {"max_angle": 120.0}
_ANGLE = {False: ("", {}), True: ("_angle", ANGLE_OPTS), "wide": ("_wide_angle", WIDE_ANGLE_OPTS)}


def pairs_sized(n, angle=False):
    """n points: a ring of close pairs at distance 0.3 around every point's partner so that the list is not empty at n = 2,
    the rest uniform.  Ragged last tile / chunk (min(lane, n_in - 1), min(pId, n_q - 1), pvalid)."""
    rng = np.random.default_rng(100 + n)
    Q = rng.uniform(-0.5, 0.5, (n, 3))
    Q[0] = (-0.15, 0.02, 0.01); Q[1] = (0.15, -0.01, 0.0)
    base = (0, 1, 0, 1) if n < 4 else (0, 1, n - 2, n - 1)
    suffix, opts = _ANGLE[angle]
    return Case("pairs_n%d%s" % (n, suffix), Q.astype(F), options=dict(opts),
                base=base, calls=((0.3, 0.0, 0.04, 0, 1), (0.45, 0.0, 0.03, 0, 1)),
                regimes={"both_orders_emitted": both_orders, "one_sided_kept": one_sided} if angle == "wide" else {})


def pairs_dense(angle=False):
    """256 + 256 cluster points: 131 072 ordered pairs, 16 384 accepted tests per tile of B."""
    return Case("pairs_dense%s" % ("_angle" if angle else ""), two_clusters(256, 256), delta=1e-4,
                options=dict(ANGLE_OPTS) if angle else {}, base=(0, 256, 1, 257), calls=((0.5, 0.0, 0.02, 0, 1),),
                regimes={"wave_own_append": lambda pairs: wave_own_append(pairs, 512, angle)})


def pairs_dense_wide_angle():
    """The 256 + 256 clusters and a base segment of length 0.5 along y (two points of its own, ids 512 and 513) under max_angle =
    120 deg: every cluster pair is parallel to x, its cosine with the segment is ~0, so every candidate of a batch emits both
    ordered pairs: 128 entries a batch, 32 768 emitted pairs per tile of B."""
    Q = np.concatenate([two_clusters(256, 256), np.array([(0.25, -0.25, 0.0), (0.25, 0.25, 0.0)], F)])
    return Case("pairs_dense_wide_angle", Q, delta=1e-4, options=dict(WIDE_ANGLE_OPTS), base=(0, 256, 512, 513),
                calls=((0.5, 0.0, 0.02, 2, 3),),
                regimes={"wave_own_append": lambda pairs: wave_own_append(pairs, 514, True), "both_orders_emitted": both_orders})


def pairs_small_radius():
    """pair_distance < eps (lo_r = max(r - E, 0)) on a cloud with exact duplicates: distance 0 is inside the band, and of a
    duplicated point's two copies only pId > j decides."""
    rng = np.random.default_rng(7)
    X = rng.uniform(-0.06, 0.06, (129, 3))
    X[90:] = X[:39]                                                   # 39 exact duplicates, ids far apart (other tiles)
    return Case("pairs_small_radius", X.astype(F), delta=1e-4, base=(0, 1, 2, 3), calls=((0.01, 0.0, 0.02, 0, 1), (0.03, 0.0, 0.02, 0, 1)),
                regimes={"duplicates_paired": lambda pairs: (all((i, 90 + i) in set(map(tuple, np.asarray(pairs).tolist())) for i in range(39)), 39)})


def pairs_attributes(n=193):
    """Normals (some zero: the filter is skipped), colours (some negative: use_rgb false), a non-zero pair_normals_angle,
    at a ragged size."""
    rng = np.random.default_rng(11)
    Q = rng.uniform(-0.5, 0.5, (n, 3))
    N = rng.normal(size=(n, 3)); N /= np.linalg.norm(N, axis=1)[:, None]
    N[rng.choice(n, n // 6, replace=False)] = 0.0
    Cc = rng.uniform(0, 1, (n, 3))
    Cc[rng.choice(n, n // 6, replace=False)] = -1.0
    Cc[:4] = (0.5, 0.5, 0.5); N[:4] = np.eye(3)[[0, 1, 2, 0]]          # the base points carry real attributes
    return Case("pairs_attributes", Q.astype(F), attrs=(N.astype(F), Cc.astype(F)),
                options={"max_normal_difference": 40.0, "max_color_distance": 0.55}, base=(0, 1, 2, 3),
                calls=((0.35, 1.2, 0.05, 0, 1), (0.5, 0.7, 0.04, 2, 3)))


def pair_cases():
    out = [pairs_sized(n, a) for n in PAIR_SIZES for a in (False, True)]
    out += [pairs_sized(513, "wide"), pairs_dense(False), pairs_dense(True), pairs_dense_wide_angle(), pairs_small_radius(), pairs_attributes()]
    return {c.name: c for c in out}


# ------------------------------------------------------------------------------------------------------------------
# quad cases (stage-level lists: the pair list of the 24 + 24 + 200 cloud, cut and repeated)
# ------------------------------------------------------------------------------------------------------------------
QUAD_EPS = 0.02


def quad_cloud(angle=False):
    return Case("quad_cloud%s" % ("_angle" if angle else ""), two_clusters(24, 24, 200, seed=3), delta=1e-4,
                options={"max_angle": 60.0} if angle else {}, base=(0, 24, 1, 25), calls=((0.5, 0.0, QUAD_EPS, 0, 1),))


def split_lists(pairs):
    """(dense, sparse): the pairs between the two clusters (ids < 48), and the rest (at least one filler), in list order."""
    p = np.asarray(pairs)
    d = (p < 48).all(1)
    return p[d], p[~d]


def _take(p, m):
    """m entries of list p, repeating it when it is shorter (lists with repeated entries)."""
    return np.ascontiguousarray(np.resize(p, (m, 2)) if len(p) < m else p[:m])


def quad_lists(pairs):
    """name -> (pairs1, pairs2, regimes) over the cluster cloud's pair list; inv1 = inv2 = 0.5, thr = QUAD_EPS."""
    dense, sparse = split_lists(pairs)
    mixed = np.ascontiguousarray(np.asarray(pairs)[::3])
    out = {}
    for m2 in QUAD_M2:                      # ragged tiles of set 2: a cut of the mixed list (dense and filler pairs interleaved)
        out["m2_%d" % m2] = (mixed[:300], _take(mixed[7:], m2), {})
    for m1 in QUAD_M1:                      # table size steps; m1 = 1024 / 1025 repeat the dense list's head (repeated entries)
        out["m1_%d" % m1] = (_take(dense[:600], m1), mixed[:257], {})
    out["repeated_set2"] = (dense[:200], _take(dense[:50], 300), {})
    out["tpp4"] = (dense[:300], dense[:60], {"threads_per_pair_4": lambda q, p2: threads_per_pair(q, p2, 4)})
    out["tpp2"] = (dense[:300], dense[:100], {"threads_per_pair_2": lambda q, p2: threads_per_pair(q, p2, 2)})
    out["tpp1"] = (dense[:300], dense[:256], {"threads_per_pair_1": lambda q, p2: threads_per_pair(q, p2, 1)})
    # one direction only: neighbouring entries of set 2 are then different pairs that match the SAME set-1 pairs, so a tag that is
    # off by one entry changes the order (in the full list (j,i) and (i,j) alternate and only one of the two ever matches)
    fwd = dense[dense[:, 0] < dense[:, 1]]
    out["direct_append"] = (dense, _take(fwd, 600), {"direct_append": direct_append_stage, "long_walk": long_walk,
                                                       "threads_per_pair_1": lambda q, p2: threads_per_pair(q, p2, 1)})
    # heavy set-1 entries next to each other between long runs of entries that find nothing: the chunked call's first ranges are
    # sized for the mean, so those that hold the heavy entries overflow and are bisected, more than once
    p1 = np.ascontiguousarray(np.concatenate([dense[:40], sparse[:400], dense[40:80], sparse[400:800]]))
    out["bisect"] = (p1, dense[:256], {"chunk_bisection": lambda q, p2, p1=p1: chunk_bisection(q, p1, CHUNK_CAP)})
    out["sparse"] = (sparse[:400], sparse[200:500], {})
    out["none"] = (sparse[:64], dense[:64], {"no_quads": lambda q, p2: (len(q) == 0, len(q))})
    return out


# ------------------------------------------------------------------------------------------------------------------
# the disc cloud: gate sizes and the fused pass (delta is the context's: eps = 2 delta)
# ------------------------------------------------------------------------------------------------------------------
DISC_RHO, DISC_SMALL, DISC_FILL = 0.058, 2, 120


def disc_case(which="dense"):
    Q, dense, sparse = disc_cloud(DISC_RHO, n_small=DISC_SMALL, n_fill=DISC_FILL)
    return Case("disc_" + which, Q, delta=0.01, base=dense if which == "dense" else sparse)


def base_stage_args(ref):
    """(d1, d2) of the base in ref, as Match4PCSBase::TryOneBase forms them; the invariants of the crossing segments."""
    bx = ref["bx"]
    d1 = float(F(np.linalg.norm(bx[0] - bx[1]))); d2 = float(F(np.linalg.norm(bx[2] - bx[3])))
    return d1, d2


def invariants(bx):
    """Closest-approach parameters of the base's two segments (what SelectQuadrilateral hands to TryOneBase), float."""
    p1, p2, q1, q2 = [np.asarray(v, np.float64) for v in bx]
    u, v, w = p2 - p1, q2 - q1, p1 - q1
    a, b, c, d, e = u @ u, u @ v, v @ v, u @ w, v @ w
    den = a * c - b * b
    return float(F((b * e - c * d) / den)), float(F((a * e - b * d) / den))


def fused_reference(ref, base, threads=8):
    """What try_base must report for the base in ref: the oracle's stages with every gated candidate verified in full."""
    m = ref["m"]
    eps = 2.0 * ref["delta"]
    d1, d2 = base_stage_args(ref)
    i1, i2 = invariants(ref["bx"])
    p1 = m.extract_pairs(d1, 0.0, eps, 0, 1)
    p2 = m.extract_pairs(d2, 0.0, eps, 2, 3)
    r = m.count_congruent_best(i1, i2, eps, p1, p2, np.asarray(base, np.int32), threads=threads)
    return dict(r, inv=(i1, i2), m1=len(p1), m2=len(p2), p1=p1, p2=p2)


def gate_lists(quads, n_q):
    """name -> quad list for try_congruent_set, cut from a dense base's quads: K in GATE_K with every third quad's third point
    moved elsewhere (the rms gate fits the first three points: such a quad fails it), and lists in which every quad is one."""
    q = np.ascontiguousarray(np.asarray(quads)[:max(GATE_K)]).copy()
    assert len(q) == max(GATE_K)
    bad = q.copy()
    bad[:, 2] = (bad[:, 2] + 37 + 13 * np.arange(len(bad))) % n_q
    mix = q.copy()
    mix[1::3] = bad[1::3]
    out = {"K%d" % k: mix[:k] for k in GATE_K}
    out["none_passes_1"] = bad[:1]
    out["none_passes_65"] = bad[:65]
    return out
