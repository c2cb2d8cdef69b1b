"""Shared pieces of tests/test_gpu_bounded_verify.py: Verify under an early-exit bound (s4p_set_best_hint) checked per candidate
against the oracle's full counts.

The contract (include/s4p_capi.h, s4p_set_best_hint): with a bound n in force a candidate whose true count EXCEEDS n keeps its
exact count, an abandoned candidate reports a lower bound, n_quads / n_verified / the checksums do not move, and the winner
does not move whenever its count exceeds n."""
import ctypes as C

import numpy as np


def hint_list(per, n_q, top=8):
    """The hints one base is run at: 1, both sides of tiled k_verify's per-tile switch (prune * 10 >= n_q), c - 1 and c for
    the `top` largest distinct oracle counts c, max + 1 and n_q.  (0, the reference run, is not in the list.)"""
    v = per[per >= 0]
    hs = {1, n_q // 10 - 1, n_q // 10, n_q}
    if len(v):
        for c in np.unique(v)[::-1][:top]:
            hs.update((int(c) - 1, int(c)))
        hs.add(int(v.max()) + 1)
    return sorted(h for h in hs if h >= 1)


def first_max(per):
    v = per[per >= 0]
    return int(np.nonzero(per == v.max())[0][0]) if len(v) else -1


def check_reference_run(r0, per0, per, quads):
    """The n = 0 run: every count is the oracle's, the winner is the first maximum."""
    assert np.array_equal(per0, per)
    assert r0.n_quads == len(quads) and r0.n_verified == int((per >= 0).sum())
    if r0.n_verified:
        assert r0.best_count == per.max() and r0.best_rank == first_max(per)
        assert list(r0.best_quad) == quads[first_max(per)].tolist()


def check_bounded(n, per, got, r, r0, what="", rank=True):
    """Assertions 1-5 of one (base, hint n) run: `per` the oracle's full counts (-1 = gated out), `got` the GPU's counts under
    the bound, r / r0 the s4p_base_result of this run and of the n = 0 run (r None: counts only).  rank: best_rank is the
    position in `per` (s4p_try_congruent_set; a fused pass ranks by its own order key)."""
    tag = "%s n=%d" % (what, n)
    per = np.asarray(per, np.int64)
    got = np.asarray(got, np.int64)
    assert got.shape == per.shape, tag
    assert np.array_equal(got < 0, per < 0), tag + ": gated-out pattern differs"
    over = per > n
    bad = np.nonzero(over & (got != per))[0]
    if len(bad):
        raise AssertionError("%s: %d candidates above the bound miscounted, first %d: gpu %d, oracle %d"
                             % (tag, len(bad), bad[0], got[bad[0]], per[bad[0]]))
    under = (per >= 0) & ~over
    assert np.all(got[under] >= 0) and np.all(got[under] <= per[under]), tag + ": an abandoned count is not a lower bound"
    if r is None:
        return
    assert (r.n_quads, r.n_verified, r.cand_checksum) == (r0.n_quads, r0.n_verified, r0.cand_checksum), tag
    v = per[per >= 0]
    if len(v) and v.max() > n:
        assert r.best_count == r0.best_count == v.max(), tag
        assert not rank or r.best_rank == first_max(per), tag
        assert list(r.best_quad) == list(r0.best_quad), tag
        assert np.array_equal(np.array(r.best_transform, np.float32).view(np.uint32),
                              np.array(r0.best_transform, np.float32).view(np.uint32)), tag
    else:
        assert r.best_count <= n, tag


def declare_async(L, BaseResult):
    """ctypes declarations of s4p_try_base_async / s4p_try_base_wait (capi.Context wraps only the synchronous s4p_try_base)."""
    L.s4p_try_base_async.restype = C.c_int32
    L.s4p_try_base_async.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_float, C.c_float]
    L.s4p_try_base_wait.restype = C.c_int32
    L.s4p_try_base_wait.argtypes = [C.c_void_p, C.POINTER(BaseResult)]


def try_base_async(ctx, base_ids, inv1, inv2):
    b = np.ascontiguousarray(base_ids, np.int32)
    ctx._chk(ctx.L.s4p_try_base_async(ctx.h, b.ctypes.data_as(C.POINTER(C.c_int32)), inv1, inv2))


def try_base_wait(ctx, BaseResult):
    r = BaseResult()
    ctx._chk(ctx.L.s4p_try_base_wait(ctx.h, C.byref(r)))
    return r
