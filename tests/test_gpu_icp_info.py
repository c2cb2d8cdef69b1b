"""The information pass on the MI355X (include/s4p_icp_info.h): the 11 sums and the 6x6 matrix against a numpy restatement
from ICP.correspondences, ICP.frame and the float32 centred target, edge sizes, no match, far coordinates, rejection,
determinism, and the state checks."""
import numpy as np
import pytest

from tests import icp_edge_cases as EC
from tests import icp_helpers as H
from tests import posegraph_helpers as PH

pytestmark = pytest.mark.gpu
DELTA = 0.004
D_BUMPY = 4 * DELTA
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


@pytest.fixture(scope="module")
def icp(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    B.build_normals()
    from super4pcs_amd import icp as I
    return I


@pytest.fixture(scope="module")
def bumpy():
    from super4pcs_amd import datasets as D
    return D.bumpy_pair(20_000, overlap=0.5, delta=DELTA, seed=11)


def restated_sums(Pc, idx, d2):
    """(sums[11], sum |term|[11]) over the pairs idx >= 0: float32 centred targets widened, every product in double."""
    p = Pc[idx[idx >= 0]].astype(np.float64)
    dd = d2[idx >= 0].astype(np.float64)
    s = np.zeros(11); a = np.zeros(11)
    s[0] = a[0] = len(p)
    s[1] = a[1] = dd.sum()
    s[2:5] = p.sum(0); a[2:5] = np.abs(p).sum(0)
    for k, (u, v) in enumerate(TRI):
        t = p[:, u] * p[:, v]
        s[5 + k] = t.sum(); a[5 + k] = np.abs(t).sum()
    return s, a


def restated_info(Pc, c, idx):
    """(Lambda, sum |term| per entry) = sum G^T G over p = double(p') + double(c)."""
    p = Pc[idx[idx >= 0]].astype(np.float64) + c.astype(np.float64)
    L = PH.info_from_points(p)
    A = np.zeros((6, 6))
    sq = (p * p).sum(0)
    for u in range(3):
        for v in range(3):
            A[u, v] = sq.sum() - sq[u] if u == v else np.abs(p[:, u] * p[:, v]).sum()
    ab = np.abs(p).sum(0)
    X = np.array([[0, ab[2], ab[1]], [ab[2], 0, ab[0]], [ab[1], ab[0], 0]])
    A[:3, 3:] = X; A[3:, :3] = X
    return L, A


def check(ctx, P, T_caller, what, idx_d2=None):
    """The sums for float(T centred) and the matrix for T; returns n."""
    c = ctx.frame()
    Pc = (P - c).astype(np.float32)
    Tc = H.to_centred(T_caller, c).astype(np.float32)
    idx, d2 = ctx.correspondences(Tc) if idx_d2 is None else idx_d2(Tc)
    gs = ctx.information_sums(Tc)
    cs, ca = restated_sums(Pc, idx, d2)
    assert gs[0] == cs[0] == np.count_nonzero(idx >= 0), (what, gs[0], cs[0])
    err = np.abs(gs - cs)
    worst = float(np.max(err[1:] / np.maximum(ca[1:], 1e-300)))
    assert np.all(err <= 1e-10 * ca), (what, gs, cs)
    # the matrix: s4p_icp_information converts T itself (double -> centred -> float); the same float T here
    info, n, rmse = ctx.information(T_caller)
    Tc2 = H.to_centred(np.asarray(T_caller, np.float64), c).astype(np.float32)
    assert np.array_equal(Tc2, Tc)
    L, A = restated_info(Pc, c, idx)
    assert n == int(cs[0])
    werr = 0.0
    if n:
        assert np.all(np.abs(info - L) <= 1e-10 * A + 0.0), (what, info, L)
        assert np.array_equal(info[3:, 3:], n * np.eye(3)) and np.array_equal(info, info.T)
        werr = float(np.max(np.abs(info - L)[A > 0] / A[A > 0]))
        assert abs(rmse - np.sqrt(cs[1] / n)) <= 1e-10 * rmse + 1e-300
    else:
        assert not info.any() and rmse == 0.0 and not gs.any()
    print("information, %s: n %d, sums max |gpu - numpy| / sum|term| %.3g, matrix %.3g" % (what, int(cs[0]), worst, werr))
    return int(cs[0])


def test_information_sums_and_matrix_are_the_restatement(icp, bumpy):
    P, Q, T_gt = bumpy
    assert len(P) <= 20_000 and len(Q) <= 20_000
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY)
    ctx.set_source(Q)
    for ang, sh in ((0.0, 0.0), (0.3, 0.002), (-1.0, 0.01)):
        n = check(ctx, P, H.motion(ang, sh) @ T_gt, "bumpy %g deg %g" % (ang, sh))
        assert n > 1000
    # no match: zeros, n = 0, OK
    far = H.motion(0.0, [50.0, 0.0, 0.0]) @ T_gt
    assert check(ctx, P, far, "no match") == 0
    ctx.close()


@pytest.fixture(scope="module")
def first_hit(icp, bumpy):
    P, Q, T_gt = bumpy
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY); ctx.set_source(Q)
    idx, _ = ctx.correspondences(H.to_centred(H.motion(0.3, 0.002) @ T_gt, ctx.frame()).astype(np.float32))
    ctx.close()
    return int(np.flatnonzero(idx >= 0)[0])


@pytest.mark.parametrize("n_q", [1, 63, 64, 65, 257, 524_289])
def test_information_at_edge_sizes(icp, bumpy, first_hit, n_q):
    """One lane, a ragged wave, one wave, one lane more, a ragged second workgroup, and one more than the 2048 x 256 lanes
    of a full launch (the grid-stride loop's second, ragged round)."""
    P, Q, T_gt = bumpy
    rng = np.random.default_rng(n_q)
    if first_hit + n_q <= len(Q):
        Qn = Q[first_hit:first_hit + n_q]
    else:
        reps = -(-n_q // len(Q))
        Qn = np.concatenate([Q] * reps)[:n_q].astype(np.float64)
        Qn[len(Q):] += rng.normal(scale=0.001, size=(n_q - len(Q), 3))
        Qn = Qn.astype(np.float32)
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY)
    ctx.set_source(Qn)
    n = check(ctx, P, H.motion(0.3, 0.002) @ T_gt, "n_Q %d" % n_q)
    assert n >= (1 if n_q < 1000 else 1000)
    ctx.close()


def test_information_at_far_coordinates(icp):
    """Coordinates around 1e4: the frame c carries the offset, and the binomial expansion in c meets sum G^T G over
    p = p' + c within the same bound."""
    case = EC.far()
    ctx = icp.ICP(0)
    ctx.set_target(case.P, case.d)
    ctx.set_source(case.Q[:30_000])
    assert np.all(np.abs(ctx.frame()) > 1e3)
    n = check(ctx, case.P, case.T0, "far")
    assert n > 1000
    ctx.close()


def test_information_under_rejection(icp, bumpy):
    from super4pcs_amd import normals
    P, Q, T_gt = bumpy
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY); ctx.set_source(Q)
    ctx.estimate_normals(D_BUMPY, 6)
    ctx.set_source_normals(normals.estimate_normals(Q, k=16))
    T = H.motion(0.5, 0.003) @ T_gt
    Tc = H.to_centred(T, ctx.frame()).astype(np.float32)
    s_off = ctx.information_sums(Tc)
    i_off = ctx.information(T)
    for kw in (dict(reciprocal=True), dict(normal_angle=60), dict(reciprocal=True, normal_angle=60)):
        ctx.set_rejection(**kw)
        n = check(ctx, P, T, "rejection %s" % (kw,), idx_d2=lambda t: ctx.rejection(t)[:2])
        counts = ctx.rejection_counts()
        assert n == counts[3] and 1000 < n < s_off[0], (kw, counts, s_off[0])
    ctx.set_rejection()
    assert ctx.information_sums(Tc).tobytes() == s_off.tobytes()
    again = ctx.information(T)
    assert again[0].tobytes() == i_off[0].tobytes() and again[1:] == i_off[1:]
    ctx.close()


def test_information_is_deterministic_and_torch_agrees(icp, bumpy):
    import torch
    P, Q, T_gt = bumpy
    T = H.motion(0.3, 0.002) @ T_gt
    ctx = icp.ICP(0)
    ctx.set_target(P, D_BUMPY); ctx.set_source(Q)
    Tc = H.to_centred(T, ctx.frame()).astype(np.float32)
    s1, s2 = ctx.information_sums(Tc), ctx.information_sums(Tc)
    a, b = ctx.information(T), ctx.information(T)
    assert s1.tobytes() == s2.tobytes() and a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    dev = torch.device("cuda:0")
    ctx2 = icp.ICP(0)
    ctx2.set_target(torch.from_numpy(P).to(dev), D_BUMPY); ctx2.set_source(torch.from_numpy(Q).to(dev))
    assert ctx2.information_sums(Tc).tobytes() == s1.tobytes()
    c2 = ctx2.information(T)
    assert c2[0].tobytes() == a[0].tobytes() and c2[1:] == a[1:]
    one = icp.information(P, Q, T, max_distance=D_BUMPY)
    assert one[0].tobytes() == a[0].tobytes() and one[1:] == a[1:]
    ctx.close(); ctx2.close()


def test_information_state_and_shared_buffers(icp, bumpy):
    P, Q, T_gt = bumpy
    ctx = icp.ICP(0)
    T32 = np.eye(4, dtype=np.float32)
    with pytest.raises(icp.ICPError) as e:
        ctx.information_sums(T32)
    assert e.value.code == -7
    ctx.set_target(P, D_BUMPY)
    for call in (lambda: ctx.information_sums(T32), lambda: ctx.information(np.eye(4))):
        with pytest.raises(icp.ICPError) as e:
            call()
        assert e.value.code == -7
    ctx.set_source(Q)
    T = H.motion(0.3, 0.002) @ T_gt
    Tc = H.to_centred(T, ctx.frame()).astype(np.float32)
    before = ctx.sums(Tc)
    s = ctx.information_sums(Tc)                                 # the first call after set_source
    assert s[0] == before[0] and abs(s[1] - before[16]) <= 1e-10 * before[16]
    assert np.all(np.abs(s[2:5] - before[4:7]) <= 1e-10 * np.abs(P - ctx.frame()).sum(0))
    ctx.information(T)
    assert ctx.sums(Tc).tobytes() == before.tobytes()            # the buffers the passes share are intact
    ctx.estimate_normals(D_BUMPY, 6)
    pb = ctx.plane_sums(Tc)
    ctx.information_sums(Tc)
    assert ctx.plane_sums(Tc).tobytes() == pb.tobytes()
    ctx.set_source(Q[:100])                                      # a new source: the next call works on it
    assert ctx.information_sums(Tc)[0] == ctx.sums(Tc)[0] <= 100
    assert ctx.L.s4p_icp_information_sums(ctx.h, None, None) == -1
    assert ctx.L.s4p_icp_information(ctx.h, None, None, None, None) == -1
    ctx.close()
