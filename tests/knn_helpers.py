"""Test-side restatement of the neighbour-list and outlier-removal contract (include/s4p_knn.h) on top of the normals
restatement (tests/normals_helpers.py): lists from the numpy lexsort brute force or from tests/normals_cpu, d2 recomputed in
numpy float32 in the contract's order, lists without self as the first k of (the k + 1 list minus the own index), the mean
neighbour distances in double in ascending order, and the clouds the tests share."""
import math

import numpy as np

from tests import apps
from tests import normals_helpers as NH

EPS = 2.0 ** -52


bits = NH.bits


def d2_of(X, Q, idx):
    """float32 d2 of every listed neighbour, dx*dx + (dy*dy + dz*dz) with dx = fl(x_j - q_x); +inf where idx is -1."""
    X = np.asarray(X, np.float32); Q = np.asarray(Q, np.float32)
    j = np.where(idx < 0, 0, idx)
    dx = X[j, 0] - Q[:, None, 0]; dy = X[j, 1] - Q[:, None, 1]; dz = X[j, 2] - Q[:, None, 2]
    d2 = (dx * dx + (dy * dy + dz * dz)).astype(np.float32)
    d2[idx < 0] = np.float32(np.inf)
    return d2


def _without_self(idx1, own, k):
    """First k of (each row of the k + 1 list minus the row's own index), -1 padded; and the counts."""
    m = idx1.shape[0]
    out = np.full((m, k), -1, np.int32)
    cnt = np.zeros(m, np.int32)
    for i in range(m):
        row = idx1[i]
        row = row[(row >= 0) & (row != own[i])][:k]
        out[i, :len(row)] = row
        cnt[i] = len(row)
    return out, cnt


def lists(knn_fn, X, k, radius=None, queries=None, exclude_self=False, own=None):
    """(idx, d2, cnt) of the contract from a neighbour-set function knn_fn(X, k, radius, queries=) -> (idx, cnt) that includes
    the point itself.  own: the cloud index of every query (exclude_self with sampled queries)."""
    X = np.asarray(X, np.float32)
    Q = X if queries is None else np.asarray(queries, np.float32)
    if exclude_self:
        own = np.arange(len(X)) if own is None else own
        idx1, _ = knn_fn(X, k + 1, radius, queries=Q)
        idx, cnt = _without_self(idx1, own, k)
    else:
        idx, cnt = knn_fn(X, k, radius, queries=Q)
    finite = np.isfinite(Q).all(1)
    idx[~finite] = -1
    cnt[~finite] = 0
    return idx, d2_of(X, Q, idx), cnt


def numpy_lists(X, k, radius=None, queries=None, exclude_self=False):
    with np.errstate(invalid="ignore"):
        return lists(NH.numpy_knn, X, k, radius, queries, exclude_self)


def cpu_lists(cpu, X, k, radius=None, sample=None, exclude_self=False, queries=None):
    """The restatement's lists of the cloud's points X[sample] (or of free queries)."""
    fn = lambda X_, k_, r_, queries: cpu.knn(X_, k_, r_, queries=queries, threads=16)      # noqa: E731
    if queries is not None:
        return lists(fn, X, k, radius, queries, False)
    sample = np.arange(len(X)) if sample is None else sample
    return lists(fn, X, k, radius, np.asarray(X, np.float32)[sample], exclude_self, own=sample)


def mean_dist(d2, cnt):
    """m_j: sqrt((double)d2) summed over the list in ascending order, in double, over cnt_j; 0 for an empty list."""
    m = np.zeros(d2.shape[0], np.float64)
    for t in range(d2.shape[1]):
        on = cnt > t
        m[on] = m[on] + np.sqrt(d2[on, t].astype(np.float64))
    nz = cnt > 0
    m[nz] = m[nz] / cnt[nz].astype(np.float64)
    return m


def sor_reference(m, std_ratio):
    """(mu, sigma, t) of the contract from the m_j with correctly rounded sums (math.fsum)."""
    n = len(m)
    mu = math.fsum(m.tolist()) / n
    var = math.fsum(((m - mu) ** 2).tolist()) / (n - 1) if n > 1 else 0.0
    sigma = math.sqrt(var)
    return mu, sigma, mu + std_ratio * sigma


def check_sor(n, k, ratio, md, stats, keep, m_ref, what):
    """The bounds, with eps = 2^-52 (twice the unit roundoff, so every "one rounding" below is covered with room):
    - m_j: k sqrt roundings, k - 1 additions and one division of non-negative terms: relative (k + 2) eps.
    - mu, t: any summation order of n non-negative terms is within relative (n - 1) eps / 2 of the exact sum; with the
      division, relative n eps.  t = mu + ratio sigma inherits it (sigma's bound below is no larger for n >= 8).
    - sigma: S = sum (m_j - mu')^2 with the device's mu' = mu (1 + theta), |theta| <= n eps.  Since sum (m_j - mu) = 0,
      sum (m_j - mu')^2 = S + n (mu - mu')^2: the error of mu enters at second order, n (n eps mu)^2.  Each term carries
      the rounding of the difference (twice, squared) and of the square, 3 eps / 2, and the sum of n non-negative terms
      (n - 1) eps / 2; the division by n - 1 and the square root add 3 eps / 2 and the root halves what came before.  In
      all |sigma' - sigma| / sigma <= (n / 4 + 4) eps + n (n eps mu)^2 / (2 S), and the same 4 eps again for the
      reference's own (m - mu)^2 terms: (n / 4 + 8) eps + (n eps mu / sigma)^2 / 2 is asserted."""
    mu, sigma, t = sor_reference(m_ref, ratio)
    rel_m = np.max(np.abs(md - m_ref) / np.where(m_ref > 0, m_ref, 1.0))
    gap = np.min(np.abs(m_ref - t)) / t if t > 0 else np.inf
    keep_ref = m_ref <= t
    print("%s: n %d k %d ratio %g: mu %.17g (ref %.17g) sigma %.17g (ref %.17g) t %.17g (ref %.17g) max rel m %.3g "
          "(equal %s) gap %.3g kept %d (ref %d)" % (what, n, k, ratio, stats["mean"], mu, stats["stddev"], sigma, stats["threshold"], t,
                                                     rel_m, np.array_equal(md, m_ref), gap, stats["kept"], keep_ref.sum()))
    assert stats["n"] == n
    assert rel_m <= (k + 2) * EPS
    assert abs(stats["mean"] - mu) <= n * EPS * mu
    assert abs(stats["threshold"] - t) <= n * EPS * t
    if sigma > 0:
        assert abs(stats["stddev"] - sigma) <= ((n / 4 + 8) * EPS + 0.5 * (n * EPS * mu / sigma) ** 2) * sigma
    else:
        assert stats["stddev"] == 0.0
    # the mask is the device's own comparison, exactly, and the reference's
    assert np.array_equal(keep, md <= stats["threshold"]) and stats["kept"] == int(keep.sum())
    assert gap > 1e-9                                    # no reference m_j so near the reference t that rounding could flip it
    assert np.array_equal(keep, keep_ref)
    return keep_ref


def plant(X, count):
    """X plus `count` points uniform in X's bounding box scaled 1.5x about its centre (default_rng(5)), the whole permuted.
    Returns (cloud float32, planted bool mask)."""
    X = np.asarray(X, np.float32)
    rng = np.random.default_rng(5)
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    c, half = 0.5 * (lo + hi), 0.75 * (hi - lo)
    extra = rng.uniform(c - half, c + half, size=(count, 3)).astype(np.float32)
    whole = np.concatenate([X, extra])
    planted = np.concatenate([np.zeros(len(X), bool), np.ones(count, bool)])
    perm = rng.permutation(len(whole))
    return np.ascontiguousarray(whole[perm]), planted[perm]


def tiny_cloud(n, dup):
    """n random points; with dup a third of them repeat earlier ones (ties at d2 = 0, broken by index)."""
    rng = np.random.default_rng(1000 + n)
    P = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    if dup and n >= 2:
        c = max(1, n // 3)
        P[n - c:] = P[rng.integers(0, n - c, c)]
    return P


TINY_N = (1, 2, 3, 8, 9, 33, 255, 256, 257)


def tiny_radius(n):
    """About half a neighbour expected within it: most lists come out short, some hold a few."""
    return np.float32(0.5 * n ** (-1.0 / 3.0))


write_obj = apps.write_obj
