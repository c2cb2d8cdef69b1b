"""Robust ICP (include/s4p_icp_robust.h) on the host: exports and binding, the loud failure without a device, the device's
radix select restated in Python against np.partition, the weight formulas, the weighted Horn solve against a weighted
Kabsch, the command line's new flags, and the facade header."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import icp_robust_helpers as RH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def icp_lib(s4p_lib_built):
    from super4pcs_amd import build as B
    B.build_icp()
    from super4pcs_amd import icp
    return icp


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(s4p_icp_\w+)\s*\(", txt)))


def test_robust_functions_are_exported_and_bound(icp_lib):
    decl = _declared("s4p_icp_robust.h")
    assert decl == sorted(icp_lib.ROBUST_SYMBOLS) and len(decl) == 3, decl
    assert not set(decl) & (set(icp_lib.SYMBOLS) | set(icp_lib.PLANE_SYMBOLS))
    L = ctypes.CDLL(icp_lib.LIB_PATH)
    assert not [s for s in decl if not hasattr(L, s)]
    Lb = icp_lib.load_library()
    for s in decl:
        assert getattr(Lb, s).argtypes is not None
    # every exported function of the library is an s4p_icp_ entry point or lives in the C++ namespace s4p_icp (the rest
    # are the sort library's weak templates)
    out = subprocess.run(["nm", "-D", "--defined-only", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    strong = [ln.split()[-1] for ln in out.splitlines() if ln.split()[-2] == "T"]
    assert strong and all(s.startswith(("s4p_icp_", "_ZN7s4p_icp")) for s in strong), strong
    assert set(decl) <= set(strong)
    dem = subprocess.run(["nm", "-C", icp_lib.LIB_PATH], capture_output=True, text=True).stdout
    for k in ("k_search", "k_key_hist", "k_key_digit", "k_wsum", "k_wfinal"):
        assert re.search(r"s4p_icp::%s\b" % k, dem), k


def test_robust_defaults_and_parameters(icp_lib):
    r = icp_lib.robust_params("huber")
    assert (r.loss, r.trim_fraction, r.scale, r.c) == (2, 1.0, 0.0, 1.345)
    r = icp_lib.robust_params("tukey", scale=0.5)
    assert (r.loss, r.scale, r.c) == (3, 0.5, 4.685)
    r = icp_lib.robust_params("trimmed", trim_fraction=0.6)
    assert (r.loss, r.trim_fraction) == (1, 0.6)
    assert ctypes.sizeof(icp_lib.Robust) == 64
    for bad in (dict(loss="trimmed"), dict(loss="trimmed", trim_fraction=0.5, scale=1.0), dict(loss="huber", trim_fraction=0.5),
                dict(loss="l1")):
        with pytest.raises(ValueError):
            icp_lib.robust_params(**bad)


def test_robust_create_without_a_gpu_fails_loudly(icp_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: creation succeeds there")
    with pytest.raises(icp_lib.ICPError) as e:
        icp_lib.ICP(0)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)


def radix_select(keys_bits, n_q, mode, kq=None):
    """k_key_hist + k_key_digit restated: 4 digits of 8 bits over the uint32 keys (0xFFFFFFFF = no key).  Returns (M, k,
    threshold bits)."""
    keys = np.asarray(keys_bits, np.uint32)
    valid = keys != np.uint32(0xFFFFFFFF)
    prefix, k, rank, M = 0, 0, 0, 0
    for p in range(4):
        shift = 24 - 8 * p
        hi = 0 if p == 0 else (0xFFFFFFFF << (shift + 8)) & 0xFFFFFFFF
        sel = valid & ((keys & np.uint32(hi)) == np.uint32(prefix & hi))
        h = np.bincount(((keys[sel] >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
        if p == 0:
            M = int(h.sum())
            k = min(M, max(1, kq)) if mode == "trim" else ((M + 1) // 2 if mode == "median" else 0)
            rank = k
        if k == 0:
            break
        b = 0
        while b < 255 and rank > h[b]:
            rank -= h[b]
            b += 1
        prefix |= b << shift
    return M, k, prefix if k else 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_radix_select_restatement_equals_np_partition_on_ties(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    u = rng.choice(np.array([0.0, 1e-30, 1e-8, 0.25, 0.5, 1.0, 3.0], np.float32), size=n)        # many ties, zeros, denormals
    u[: n // 3] = rng.uniform(0, 2e-3, n // 3).astype(np.float32) ** 2
    u[n // 3: n // 3 + 50] = u[0]                                                               # duplicates of one value
    bits = u.view(np.uint32).copy()
    bits[rng.choice(n, 700, replace=False)] = 0xFFFFFFFF                                         # misses
    keyed = bits != 0xFFFFFFFF
    uk = bits[keyed].view(np.float32)
    M = len(uk)
    for k in (1, 2, M // 3, M // 2, M - 1, M):
        _, kk, thr = radix_select(bits, n, "trim", kq=k)
        assert kk == k and thr == int(RH.select(uk, k).view(np.uint32))
    Mm, kk, thr = radix_select(bits, n, "median")
    assert Mm == M and kk == (M + 1) // 2 and thr == int(RH.select(uk, kk).view(np.uint32))
    assert radix_select(bits, n, "trim", kq=10 * n)[1] == M                                     # k capped at M
    assert radix_select(np.full(10, 0xFFFFFFFF, np.uint32), 10, "median") == (0, 0, 0)
    assert radix_select(np.zeros(10, np.uint32), 10, "median") == (10, 5, 0)                   # exact fit: every key 0
    same = np.full(100, np.float32(0.125)).view(np.uint32)
    assert radix_select(same, 100, "trim", kq=30)[2] == int(same[0])


def test_weight_formulas_are_the_contract():
    u = np.array([0.0, 1.0, 4.0, 9.0, 16.0, 25.0], np.float32)
    # trimmed: u <= u_(k), ties included
    k, thr, s = RH.scale_and_k(np.array([1, 2, 2, 2, 3], np.float32), "trimmed", 5, 1.0, trim_fraction=0.4)
    assert (k, float(thr), s) == (2, 2.0, 0.0)
    assert RH.weights(np.array([1, 2, 2, 2, 3], np.float32), "trimmed", thr, s).tolist() == [1, 1, 1, 1, 0]
    # Huber with c s = 2: w = 1 up to u = 4, then 2 / sqrt(u)
    w = RH.weights(u, "huber", None, 2.0, c=1.0)
    assert w.tolist() == [1.0, 1.0, 1.0, 2 / 3, 0.5, 0.4]
    # Tukey with c s = 4: (1 - u / 16)^2 below 16, 0 from 16 on
    w = RH.weights(u, "tukey", None, 4.0, c=1.0)
    assert w.tolist() == [1.0, (15 / 16) ** 2, (12 / 16) ** 2, (7 / 16) ** 2, 0.0, 0.0]
    # the estimated scale: 1.4826 sqrt(u_(ceil(M/2))), at least 1e-6 max_distance
    k, thr, s = RH.scale_and_k(u, "tukey", 6, 0.5)
    assert k == 3 and float(thr) == 4.0 and s == 1.4826 * 2.0
    k, thr, s = RH.scale_and_k(np.zeros(7, np.float32), "huber", 7, 0.5)
    assert k == 4 and float(thr) == 0.0 and s == 1e-6 * 0.5
    assert RH.scale_and_k(u, "huber", 6, 0.5, scale=0.25) == (0, None, 0.25)
    # trimmed k = min(M, max(1, ceil(xi n_Q)))
    assert RH.scale_and_k(u, "trimmed", 100, 1.0, trim_fraction=0.001)[0] == 1
    assert RH.scale_and_k(u, "trimmed", 100, 1.0, trim_fraction=0.5)[0] == 6
    assert RH.scale_and_k(u, "trimmed", 10, 1.0, trim_fraction=0.21)[0] == math.ceil(0.21 * 10)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_weighted_horn_solve_equals_a_weighted_kabsch(icp_lib, seed):
    rng = np.random.default_rng(seed)
    n = 400
    q = rng.normal(size=(n, 3)) * np.array([1.0, 0.7, 0.4])
    A = rng.normal(size=(3, 3)); U, _, Vt = np.linalg.svd(A); R = U @ Vt
    if np.linalg.det(R) < 0:
        R[:, 0] *= -1
    t = rng.normal(size=3)
    p = q @ R.T + t + rng.normal(scale=1e-2, size=q.shape)
    w = rng.uniform(0, 1, n) ** 2
    w[::7] = 0.0
    s = np.zeros(17)
    s[0] = w.sum(); s[1:4] = (q * w[:, None]).sum(0); s[4:7] = (p * w[:, None]).sum(0)
    s[7:16] = ((q * w[:, None]).T @ p).reshape(9); s[16] = 1.0
    got = icp_lib.solve(s)
    mq = (q * w[:, None]).sum(0) / w.sum(); mp = (p * w[:, None]).sum(0) / w.sum()
    H = ((q - mq) * w[:, None]).T @ (p - mp)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    Rk = Vt.T @ D @ U.T
    want = np.eye(4); want[:3, :3] = Rk; want[:3, 3] = mp - Rk @ mq
    assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), np.max(np.abs(got - want))


def test_robust_restatement_with_unit_weights_is_the_plain_restatement():
    """trimmed with xi = 1 and Huber with a huge fixed scale weight every pair 1: the plain sums come back."""
    from tests import icp_helpers as H
    from tests import icp_plane_helpers as PH
    rng = np.random.default_rng(5)
    Pc = rng.uniform(-0.5, 0.5, (1500, 3)).astype(np.float32)
    Qc = (Pc[rng.integers(0, 1500, 600)] + rng.normal(scale=0.01, size=(600, 3))).astype(np.float32)
    N = PH.normalise(rng.normal(size=Pc.shape)); N[::9] = 0
    T = np.eye(4); T[:3, 3] = [0.003, -0.002, 0.001]
    idx, d2 = H.numpy_brute(Pc, Qc, T, 0.04)
    plain = PH.plane_sums(Pc, Qc, T, idx, d2, N)
    for kw in (dict(loss="trimmed", trim_fraction=1.0), dict(loss="huber", scale=1e3)):
        s, info = RH.robust_sums(Pc, Qc, T, idx, d2, "plane", n_q=600, d=0.04, Nc=N, **kw)
        assert np.allclose(s, plain, rtol=1e-12, atol=1e-15) and info[4] == plain[0] and s[2] == plain[2]
        sp, infop = RH.robust_sums(Pc, Qc, T, idx, d2, "point", n_q=600, d=0.04, **kw)
        assert sp[0] == infop[4] == np.count_nonzero(idx >= 0)


def test_cli_icp_loss_flags_parse_and_bad_values_exit_with_usage(s4p_lib_built, tmp_path):
    from super4pcs_amd import build as B
    cli = B.build_cli()
    for bad in (["--icp-loss", "l1"], ["--icp-loss", ""], ["--icp-loss", "trimmed", "--icp-trim", "0"],
                ["--icp-loss", "trimmed", "--icp-trim", "1.5"], ["--icp-loss", "trimmed", "--icp-trim", "nan"],
                ["--icp-loss", "trimmed", "--icp-trim", "0.5x"], ["--icp-loss", "huber", "--icp-loss-scale", "0"],
                ["--icp-loss", "tukey", "--icp-loss-scale", "-1"], ["--icp-loss", "tukey", "--icp-loss-scale", "inf"],
                ["--icp-trim", "0.5"], ["--icp-loss", "none", "--icp-trim", "0.5"], ["--icp-loss", "huber", "--icp-trim", "0.5"],
                ["--icp-loss-scale", "0.1"], ["--icp-loss", "trimmed", "--icp-loss-scale", "0.1"]):
        r = subprocess.run([cli, "-i", "a.obj", "b.obj", "--icp", "30"] + bad, capture_output=True, text=True)
        assert r.returncode == 1 and "Usage:" in r.stderr and "--icp-loss" in r.stderr, (bad, r.returncode, r.stderr)
    for good in (["--icp-loss", "trimmed"], ["--icp-loss", "trimmed", "--icp-trim", "0.6"], ["--icp-trim", "1", "--icp-loss", "trimmed"],
                 ["--icp-loss", "huber"], ["--icp-loss", "tukey", "--icp-loss-scale", "0.02"], ["--icp-loss", "none"],
                 ["--icp-loss", "huber", "--icp-metric", "plane"]):
        r = subprocess.run([cli, "-i", str(tmp_path / "none1.obj"), str(tmp_path / "none2.obj"), "--icp", "30"] + good,
                           capture_output=True, text=True)
        assert r.returncode == 255 and "Can't read input set1" in r.stderr, (good, r.stderr)


def test_facade_header_with_robust_options_compiles(tmp_path):
    src = tmp_path / "robust_facade.cpp"
    src.write_text('#include "super4pcs/algorithms/icp.h"\n'
                   "using namespace GlobalRegistration;\n"
                   "int main() {\n"
                   "  ICPOptions o;\n"
                   "  static_assert(sizeof(s4p_icp_robust) == 64, \"abi\");\n"
                   "  const bool plain = o.loss == ICPLoss::None && o.trim_fraction == 1.0 && o.loss_scale < 0;\n"
                   "  o.loss = ICPLoss::Tukey; o.loss = ICPLoss::Huber; o.loss = ICPLoss::Trimmed; o.trim_fraction = 0.6;\n"
                   "  return plain ? 0 : 1;\n"
                   "}\n")
    for extra in ([], ["-DS4P_USE_EIGEN=0"]):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + extra +
                           [str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
