"""Test-side restatement of the normal-orientation contract (include/s4p_normals_orient.h) in numpy and plain Python: the
edge weights in float32 term by term, Kruskal under the contract's strict order (bits of w, min(i, j), max(i, j)), the anchor
of every tree, and a walk of the tree from it.  The lists come from tests/knn_helpers.py (the numpy brute force or
tests/normals_cpu).  Nothing here follows the device path: no Boruvka rounds, no pointer jumping."""
import numpy as np

from tests import knn_helpers as KH
from tests import normals_helpers as NH

bits = NH.bits


def usable(N):
    """The vertices: normals whose components are finite and not all zero."""
    N = np.asarray(N, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(N).all(1) & (N != 0).any(1)


def dot(A, B):
    """ax*bx + (ay*by + az*bz) in float32, term by term."""
    A = np.asarray(A, np.float32); B = np.asarray(B, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (A[..., 0] * B[..., 0] + (A[..., 1] * B[..., 1] + A[..., 2] * B[..., 2])).astype(np.float32)


def edges(N, idx):
    """The undirected edges of the contract: (lo, hi, w float32, f bool), each pair once, in no particular order."""
    N = np.asarray(N, np.float32)
    n, k = idx.shape
    ok = usable(N)
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    j = idx.reshape(-1).astype(np.int64)
    keep = (j >= 0) & ok[i] & ok[np.where(j < 0, 0, j)]
    i, j = i[keep], j[keep]
    code = np.unique(np.minimum(i, j) * n + np.maximum(i, j))
    lo, hi = code // n, code % n
    d = dot(N[lo], N[hi])
    with np.errstate(invalid="ignore"):
        t = (np.float32(1) - np.abs(d)).astype(np.float32)
        w = np.where(t > 0, t, np.float32(0)).astype(np.float32)
        f = d < 0
    return lo, hi, w, f


def reference(X, N, idx, viewpoint=None):
    """(flip bool[n], component int32[n], components): the contract on the lists idx (rows without the own index)."""
    X = np.ascontiguousarray(X, np.float32); N = np.ascontiguousarray(N, np.float32)
    n = len(X)
    ok = usable(N)
    lo, hi, w, f = edges(N, idx)
    order = np.lexsort((hi, lo, bits(w)))
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    adj = [[] for _ in range(n)]
    for a, b, fl in zip(lo[order].tolist(), hi[order].tolist(), f[order].tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
            adj[a].append((b, fl)); adj[b].append((a, fl))
    root = np.array([find(v) if ok[v] else -1 for v in range(n)], np.int64)
    if viewpoint is None:
        p = (np.float32(0.5) * (X.min(0) + X.max(0))).astype(np.float32)
    else:
        p = np.asarray(viewpoint, np.float32)
    with np.errstate(over="ignore"):
        dx = X[:, 0] - p[0]; dy = X[:, 1] - p[1]; dz = X[:, 2] - p[2]
        d2 = (dx * dx + (dy * dy + dz * dz)).astype(np.float32)
    flip = np.zeros(n, bool)
    comp = np.full(n, -1, np.int32)
    seen = np.zeros(n, bool)
    ncomp = 0
    for r in np.unique(root[root >= 0]):
        mem = np.flatnonzero(root == r)
        key = bits(d2[mem]).astype(np.int64)
        a = int(mem[np.lexsort((mem, key if viewpoint is not None else -key))[0]])
        g = (p - X[a]) if viewpoint is not None else (X[a] - p)
        flip[a] = bool(dot(N[a], g.astype(np.float32)) < 0)
        ncomp += 1
        seen[a] = True
        stack = [a]
        while stack:
            u = stack.pop()
            comp[u] = a
            for v, fl in adj[u]:
                if not seen[v]:
                    seen[v] = True
                    flip[v] = flip[u] ^ fl
                    stack.append(v)
    assert np.array_equal(seen, ok)
    return flip, comp, ncomp


def apply(N, flip):
    """The normals with the flipped rows negated (the sign bit of every component, zeros included)."""
    out = np.array(N, np.float32, copy=True)
    out[flip] = -out[flip]
    return out


def towards(X, N, viewpoint):
    """s4p_orient_towards in one expression: flip = usable & (n . fl(v - x) < 0)."""
    X = np.asarray(X, np.float32); N = np.asarray(N, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        flip = usable(N) & (dot(N, np.asarray(viewpoint, np.float32)[None, :] - X) < 0)
    return apply(N, flip), flip


def pca_normals(X, idx):
    """Unoriented normals in numpy: the eigenvector of the smallest eigenvalue of each list's covariance (double), signed
    as the library signs its estimates (the component of largest magnitude positive)."""
    P = np.asarray(X, np.float64)
    nb = P[idx]
    e = nb - nb.mean(1, keepdims=True)
    Cm = np.einsum("nki,nkj->nij", e, e)
    v = np.linalg.eigh(Cm)[1][:, :, 0]
    lead = v[np.arange(len(v)), np.abs(v).argmax(1)]
    return (v * np.where(lead < 0, -1.0, 1.0)[:, None]).astype(np.float32)


def lattice(m, seed=0):
    """An m x m planar lattice with normals +-z of random sign: every edge weight is 0, every decision a tie-break."""
    g = np.arange(m, dtype=np.float32) * np.float32(0.125)
    X = np.column_stack([np.repeat(g, m), np.tile(g, m), np.zeros(m * m, np.float32)]).astype(np.float32)
    rng = np.random.default_rng(seed + m)
    N = np.zeros((m * m, 3), np.float32)
    N[:, 2] = np.where(rng.random(m * m) < 0.5, -1.0, 1.0)
    return X, N


def random_normals(n, seed, zeros=True):
    """Random unit normals; with zeros, about a tenth of them (0, 0, 0) (at least one when n >= 3)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    N = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    if zeros and n >= 3:
        z = rng.random(n) < 0.1
        z[rng.integers(0, n)] = True
        N[z] = 0
    return N


def two_clusters(n_each=150, seed=4):
    """Two noisy sphere caps far apart (centres at x = -10 and x = +10, radius 1), with radial normals of random sign: two
    components at any k < n_each.  Returns (X, N, centre of each point's cluster)."""
    rng = np.random.default_rng(seed)
    out, nrm, ctr = [], [], []
    for cx in (-10.0, 10.0):
        d = rng.normal(size=(n_each, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        c = np.array([cx, 0.0, 0.0])
        out.append(c + d); nrm.append(d * np.where(rng.random(n_each) < 0.5, -1.0, 1.0)[:, None]); ctr.append(np.tile(c, (n_each, 1)))
    perm = rng.permutation(2 * n_each)
    return (np.concatenate(out)[perm].astype(np.float32), np.concatenate(nrm)[perm].astype(np.float32), np.concatenate(ctr)[perm])


def same(ctx, X, N, idx, k, radius, viewpoint, what):
    """One orient call equals the restatement: mask, components, counts, and the output's bits.  Returns the info."""
    out, info = ctx.orient(N, k, radius, viewpoint, return_info=True)
    flip, comp, ncomp = reference(X, N, idx, viewpoint)
    assert out.dtype == np.float32 and info["flipped"].dtype == bool and info["component"].dtype == np.int32
    bad = np.flatnonzero(info["flipped"] != flip)
    assert len(bad) == 0, (what, len(bad), bad[:8])
    assert np.array_equal(info["component"], comp), (what, np.flatnonzero(info["component"] != comp)[:8])
    assert np.array_equal(bits(out), bits(apply(N, flip))), what
    assert (info["vertices"], info["components"], info["flipped_count"]) == (int(usable(N).sum()), ncomp, int(flip.sum())), (what, info)
    assert 0 <= info["rounds"] <= 32 and 0 <= info["max_jumps"] <= 32 and (info["rounds"] == 0) == (info["max_jumps"] == 0)
    return info


numpy_lists = KH.numpy_lists
cpu_lists = KH.cpu_lists
