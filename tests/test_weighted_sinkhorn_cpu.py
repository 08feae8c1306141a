"""CPU tier of the weighted-marginal Sinkhorn solver and loss (include/kccot_weighted.h,
gan_utils.compute_weighted_sinkhorn / compute_weighted_sinkhorn_loss): the float64 yardstick the GPU tier
(tests/test_gpu_weighted_sinkhorn.py) is held to, proved here against the project's own oracle, plus the header, the ctypes
table and the argument validation of the new entry points.

The yardstick is the weighted loop in plain torch float64, unrolled, with autograd through it:

    u = v = 0; repeat up to L times (count-based stop, Lmin = 100, thresh 1e-2):
        u_i += eps (log a_i - LSE_j((-C_ij + u_i + v_j)/eps))
        v_j += eps (log b_j - LSE_i((-C_ij + u_i + v_j)/eps))
    W(C; a, b) = sum_ij exp((-C_ij + u_i + v_j)/eps) C_ij
    loss = 2 W(C_xy; a, b) - W(C_xx; a, a) - W(C_yy; b, b)
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import torch

import cases
from oracle import gan_utils_np as onp
from oracle import gan_utils_torch as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
THRESH, LMIN = 1e-2, 100


# ================================================================ the float64 yardstick
def weighted_sinkhorn(C, a, b, eps, L, Lmin=LMIN):
    """(cost, nits, pi) of the weighted loop on C [n,n] with marginals a (rows) and b (columns); float64 torch tensors,
    differentiable w.r.t. C."""
    la, lb = torch.log(a), torch.log(b)
    u = torch.zeros_like(a)
    v = torch.zeros_like(b)
    nits = 0
    for _ in range(int(L)):
        u1 = u
        u = eps * (la - torch.logsumexp((-C + u[:, None] + v[None, :]) / eps, dim=1)) + u
        v = eps * (lb - torch.logsumexp((-C + u[:, None] + v[None, :]) / eps, dim=0)) + v
        nits += 1
        if THRESH > float((u - u1).detach().abs().sum()) and nits >= Lmin:
            break
    pi = torch.exp((-C + u[:, None] + v[None, :]) / eps)
    return (pi * C).sum(), nits, pi


def weighted_loss(real, fake, sc, eps, L, h_fake, m_real, h_real, m_fake, a, b):
    """(loss, (xy, xx, yy), nits) with the three modified_cost matrices of compute_sinkhorn_loss; videos [B, K] or any
    [B, ...], features [B,T,J], float64."""
    x, y = real.reshape(real.shape[0], 1, -1), fake.reshape(fake.shape[0], 1, -1)
    xy, n0, _ = weighted_sinkhorn(ot.modified_cost(x, y, h_fake, m_real, sc), a, b, eps, L)
    xx, n1, _ = weighted_sinkhorn(ot.modified_cost(x, x, h_real, m_real, sc), a, a, eps, L)
    yy, n2, _ = weighted_sinkhorn(ot.modified_cost(y, y, h_fake, m_fake, sc), b, b, eps, L)
    return 2.0 * xy - xx - yy, (xy, xx, yy), (n0, n1, n2)


def random_weights(n, seed):
    """softmax(2 randn): positive, normalised, spanning roughly two orders of magnitude."""
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(2.0 * torch.randn(n, generator=g, dtype=F64), dim=0)


def small_cost(n, seed, sc=1.0):
    """cost_xy of small random videos [n, 3, 4] in U[0,1): entries O(1), so the loop has work to do at eps ~ 1.  Returned
    as float32 (what the device reads)."""
    rng = np.random.default_rng(seed)
    x, y = rng.random((n, 3, 4)), rng.random((n, 3, 4))
    return torch.from_numpy(onp.cost_xy(x, y, sc, dtype=np.float64).astype(np.float32))


# ================================================================ the yardstick against the project's oracle
def test_uniform_weights_reproduce_the_oracle_compute_sinkhorn():
    shape, seed, regime = cases.CASES[2]                      # ("small", 0, "near")
    inp = cases.gen_inputs(shape, seed, regime)
    x, y = onp.flatten_video(inp["real"]), onp.flatten_video(inp["fake"])
    for eps, L in ((1.0, 100), (0.8, 200)):
        want, nits, C = onp.compute_sinkhorn_ex(x, y, inp["h_fake"], inp["m_real"], cases.SC, epsilon=eps, L=L,
                                                dtype=np.float64)
        n = C.shape[0]
        uni = torch.full((n,), 1.0 / n, dtype=F64)
        got, got_nits, _ = weighted_sinkhorn(torch.from_numpy(C), uni, uni, eps, L)
        assert got_nits == nits
        assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want)), (eps, L, float(got), float(want))


def test_uniform_weighted_loss_reproduces_the_oracle_loss():
    shape, seed, regime = cases.CASES[0]                      # ("tiny", 0, "near")
    inp = {k: torch.from_numpy(v).double() for k, v in cases.gen_inputs(shape, seed, regime).items()}
    B = inp["real"].shape[0]
    uni = torch.full((B,), 1.0 / B, dtype=F64)
    got, _, _ = weighted_loss(inp["real"], inp["fake"], cases.SC, 1.0, 100, inp["h_fake"], inp["m_real"], inp["h_real"],
                              inp["m_fake"], uni, uni)
    want = onp.compute_sinkhorn_loss(*(inp[k].numpy() for k in ("real", "fake")), cases.SC, 1.0, 100,
                                     *(inp[k].numpy() for k in ("h_fake", "m_real", "h_real", "m_fake")), dtype=np.float64)
    assert abs(float(got) - float(want)) <= 1e-11 * max(abs(float(want)), 1.0)


def test_marginals_of_the_final_plan():
    """The last half-step is the v-update, so the plan's column sums are b to float64 round-off; its row sums are off a
    by the Sinkhorn residual, which is what the u-update that would come next changes u by: |row_i - a_i| <= a_i
    (exp(|du_i|/eps) - 1)."""
    for n, seed, eps, L in ((5, 0, 1.0, 7), (16, 1, 0.8, 100), (67, 2, 1.0, 100)):
        C = small_cost(n, seed).double()
        a, b = random_weights(n, 10 + seed), random_weights(n, 20 + seed)
        _, nits, pi = weighted_sinkhorn(C, a, b, eps, L)
        assert nits == L
        assert float((pi.sum(0) - b).abs().max()) <= 1e-13
        assert abs(float(pi.sum()) - 1.0) <= 1e-13
        rows = pi.sum(1)
        du = eps * (torch.log(a) - torch.log(rows))            # the next u-update
        assert bool(((rows - a).abs() <= a * torch.expm1(du.abs() / eps) * (1 + 1e-9) + 1e-15).all())
        if L == 100:
            assert float((rows - a).abs().max()) <= 1e-6      # converged: the residual is small


def test_weights_matter_and_uniform_is_a_special_case():
    n = 16
    C = small_cost(n, 3).double()
    uni = torch.full((n,), 1.0 / n, dtype=F64)
    a, b = random_weights(n, 1), random_weights(n, 2)
    w_uni = float(weighted_sinkhorn(C, uni, uni, 1.0, 100)[0])
    w_ab = float(weighted_sinkhorn(C, a, b, 1.0, 100)[0])
    w_ba = float(weighted_sinkhorn(C, a, b[torch.randperm(n, generator=torch.Generator().manual_seed(0))], 1.0, 100)[0])
    assert abs(w_ab - w_uni) > 1e-3 * abs(w_uni) and abs(w_ab - w_ba) > 1e-3 * abs(w_ab)
    want, _ = ot.sinkhorn_from_cost(C, 1.0, 100)
    assert abs(w_uni - float(want)) <= 1e-12 * abs(float(want))


def test_gradient_of_the_yardstick_matches_finite_differences():
    n = 6
    C = small_cost(n, 4).double().requires_grad_(True)
    a, b = random_weights(n, 3), random_weights(n, 4)
    cost, _, _ = weighted_sinkhorn(C, a, b, 1.0, 12)
    (g,) = torch.autograd.grad(cost, C)
    h = 1e-6
    for i, j in ((0, 0), (2, 5), (5, 1)):
        Cp, Cm = C.detach().clone(), C.detach().clone()
        Cp[i, j] += h
        Cm[i, j] -= h
        fd = (float(weighted_sinkhorn(Cp, a, b, 1.0, 12)[0]) - float(weighted_sinkhorn(Cm, a, b, 1.0, 12)[0])) / (2 * h)
        assert abs(fd - float(g[i, j])) <= 1e-7 * max(1.0, abs(fd))


# ================================================================ header, ctypes table, argument validation
def _decls():
    text = open(os.path.join(ROOT, "include", "kccot_weighted.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_is_strict_c99_and_matches_the_ctypes_table(tmp_path):
    from kccotgan_amd import _lib
    decls = _decls()
    assert sorted(decls) == sorted(_lib.WEIGHTED_SIGNATURES), "ctypes table and header disagree"
    assert not set(_lib.WEIGHTED_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.MODEL_SIGNATURES))
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "unsigned": ctypes.c_uint,
             "size_t": ctypes.c_size_t}
    for name, args in decls.items():
        assert hasattr(_lib.lib, name), "libkccot.so does not export %s" % name
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        assert _lib.WEIGHTED_SIGNATURES[name][1] == want, name
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_weighted.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(probe), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_happens_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is rejected on its arguments
    fwd, bwd = lib.kccot_sinkhorn_weighted_fwd_f32, lib.kccot_sinkhorn_weighted_bwd_f32
    assert fwd(one, None, one, 1, 8, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EINVAL
    assert b"weight" in lib.kccot_last_error()
    assert fwd(one, one, None, 1, 8, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EINVAL
    assert fwd(None, one, one, 1, 8, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EINVAL
    assert fwd(one, one, one, 1, 0, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EINVAL
    assert fwd(one, one, one, 0, 8, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EINVAL
    assert fwd(one, one, one, 1, 8, 0.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EINVAL
    assert fwd(one, one, one, 1, 4096, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, None, 0, None) == _lib.EUNSUPPORTED
    need = lib.kccot_sinkhorn_workspace_bytes(1, 130)
    assert need > 0
    assert fwd(one, one, one, 1, 130, 1.0, 10, 10, 0.01, 0, None, None, one, one, None, one, need - 1, None) == _lib.EWORKSPACE
    assert bwd(one, None, one, one, one, one, 1, 8, 1.0, 10, one, one, None, 0, None) == _lib.EINVAL
    assert bwd(one, one, None, one, one, one, 1, 8, 1.0, 10, one, one, None, 0, None) == _lib.EINVAL
    assert bwd(one, one, one, one, one, one, 1, 0, 1.0, 10, one, one, None, 0, None) == _lib.EINVAL
    assert bwd(one, one, one, one, one, one, 1, 130, 1.0, 10, one, one, one, need - 1, None) == _lib.EWORKSPACE
    B, K = 8, 64
    lneed = lib.kccot_weighted_sinkhorn_loss_workspace_bytes(B, K)
    assert lneed >= lib.kccot_sinkhorn_loss_workspace_bytes(B, K) > 0
    assert lib.kccot_weighted_sinkhorn_loss_workspace_bytes(0, K) == 0

    def lfwd(w_real=one, w_fake=one, B=B, ws_bytes=lneed, C3=one):
        return lib.kccot_weighted_sinkhorn_loss_fwd_f32(one, one, B, K, 1.0, one, one, one, one, 4, 3, 1.0, 10, 10, 0.01, 0,
                                                        w_real, w_fake, C3, None, None, one, one, one, one, one, ws_bytes, None)

    def lbwd(w_real=one, w_fake=one, B=B, ws_bytes=lneed):
        return lib.kccot_weighted_sinkhorn_loss_bwd_f32(one, one, one, B, K, 1.0, one, one, one, one, 4, 3, 1.0, 10, w_real,
                                                        w_fake, one, one, one, one, one, None, None, None, None, one, ws_bytes,
                                                        None)

    for f in (lfwd, lbwd):
        assert f(w_real=None) == _lib.EINVAL and f(w_fake=None) == _lib.EINVAL
        assert f(B=0) == _lib.EINVAL
        assert f(ws_bytes=lneed - 1) == _lib.EWORKSPACE
    assert lfwd(C3=None) == _lib.EINVAL


def test_python_wrappers_are_exported_and_refuse_what_they_cannot_do():
    import inspect
    import pytest
    from kccotgan_amd import gan_utils as g, _lib
    assert "compute_weighted_sinkhorn" in g.__all__ and "compute_weighted_sinkhorn_loss" in g.__all__
    assert list(inspect.signature(g.compute_weighted_sinkhorn).parameters) == [
        "x", "y", "hy", "Mx", "scaling_coef", "mu", "nu", "epsilon", "L"]
    p = inspect.signature(g.compute_weighted_sinkhorn_loss).parameters
    assert list(p) == ["f_real", "f_fake", "scaling_coef", "sinkhorn_eps", "sinkhorn_l", "h_fake", "m_real", "h_real",
                       "m_fake", "w_real", "w_fake", "video", "normalize"]
    assert p["video"].default is True and p["normalize"].default is True
    x, f, w = torch.zeros(2, 3, 4), torch.zeros(2, 3, 2), torch.full((2,), 0.5)
    with pytest.raises(_lib.KccotError):                       # no CPU path
        g.compute_weighted_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w, w, video=False)
