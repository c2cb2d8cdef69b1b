"""A second copy of each library bound in the same process (Shape(0, lib=path), ICP(0, lib=path)) on the MI355X: it returns the
bits of the package's library, through a CDLL of its own, and leaves the package's cached library as it was."""
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bytes(arrays):
    return [(a.dtype.str, a.shape, np.ascontiguousarray(a).tobytes()) for a in arrays]


def test_a_copy_of_the_normals_library_next_to_the_package_s(tmp_path):
    from super4pcs_amd import build, normals, shape
    build.build_normals()
    before = normals.load_library()
    copy = shutil.copy(normals.LIB_PATH, str(tmp_path / "libsuper4pcs_normals.so"))
    X = np.random.default_rng(1).uniform(0, 1, size=(1000, 3)).astype(np.float32)
    got = []
    ctxs = [shape.Shape(0, lib=copy), shape.Shape(0)]
    for ctx in ctxs:
        ctx.set_cloud(X)
        N, eig, count = ctx.estimate(0.1)
        assert N.shape == eig.shape == (1000, 3) and count.shape == (1000,) and count.max() >= 3 and N.any()
        got.append(_bytes((N, eig, count)))
        ctx.close()
    assert got[0] == got[1]
    assert ctxs[0].L is not ctxs[1].L and ctxs[1].L is before
    assert normals.load_library() is before and shape.load_library() is before


def test_a_copy_of_the_icp_library_next_to_the_package_s(tmp_path):
    from super4pcs_amd import build, icp
    build.build_icp()
    before = icp.load_library()
    copy = shutil.copy(icp.LIB_PATH, str(tmp_path / "libsuper4pcs_icp.so"))
    rng = np.random.default_rng(2)
    P = rng.uniform(0, 1, size=(500, 3)).astype(np.float32)
    Q = (P[rng.permutation(500)] + rng.normal(0, 0.01, size=(500, 3))).astype(np.float32)
    got = []
    ctxs = [icp.ICP(0, lib=copy), icp.ICP(0)]
    for ctx in ctxs:
        ctx.set_target(P, 0.1)
        ctx.set_source(Q)
        s = ctx.sums(np.eye(4))
        assert s.shape == (icp.NSUMS,) and s[0] > 0
        got.append(_bytes((s,)))
        ctx.close()
    assert got[0] == got[1]
    assert ctxs[0].L is not ctxs[1].L and ctxs[1].L is before
    assert icp.load_library() is before
