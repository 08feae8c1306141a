"""CPU tier of the kernel-conditional Sinkhorn loss (include/kccot_conditional.h, gan_utils.kernel_conditional_weights /
compute_conditional_sinkhorn_loss): the float64 yardsticks the GPU tier (tests/test_gpu_conditional_sinkhorn.py) is held to,
proved here against the weighted yardstick of tests/test_weighted_sinkhorn_cpu.py, plus the header, the ctypes table and the
argument validation of the new entry points.

    loss = sum_q omega_q (2 W(C_xy; w_q, w_q) - W(C_xx; w_q, w_q) - W(C_yy; w_q, w_q)),   omega = 1/Q unless given
    w_qi = max(softmax_i(-D_qi / (2 bw^2)), 2^-100)
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import test_weighted_sinkhorn_cpu as W
from test_weighted_sinkhorn_cpu import F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_W = 2.0 ** -100
COEF = (2.0, -1.0, -1.0)


# ================================================================ the float64 yardsticks
def query_weights(omega, Q):
    return torch.full((Q,), 1.0 / Q, dtype=F64) if omega is None else omega.double()


def conditional_costs(C3, w, eps, L):
    """costs [Q,3] (a list of lists of float64 scalars, differentiable w.r.t. C3) and counts [Q][3] of the 3 Q weighted solves:
    problem (q, k) is W.weighted_sinkhorn on C3[k] with both marginals w[q]."""
    costs, nits = [], []
    for q in range(w.shape[0]):
        row = [W.weighted_sinkhorn(C3[k], w[q], w[q], eps, L) for k in range(3)]
        costs.append([r[0] for r in row])
        nits.append([r[1] for r in row])
    return costs, nits


def conditional_loss_from_costs(C3, w, omega, eps, L):
    """(loss, costs [Q,3], counts) on given cost matrices C3 [3,n,n], weight rows w [Q,n], omega [Q] or None; float64."""
    costs, nits = conditional_costs(C3, w, eps, L)
    om = query_weights(omega, w.shape[0])
    loss = sum(om[q] * (2.0 * c[0] - c[1] - c[2]) for q, c in enumerate(costs))
    return loss, costs, nits


def conditional_loss(real, fake, sc, eps, L, h_fake, m_real, h_real, m_fake, w, omega=None):
    """sum_q omega_q W.weighted_loss(..., a = b = w_q): the loss from videos and features, float64."""
    om = query_weights(omega, w.shape[0])
    return sum(om[q] * W.weighted_loss(real, fake, sc, eps, L, h_fake, m_real, h_real, m_fake, w[q], w[q])[0]
               for q in range(w.shape[0]))


def conditional_weights(D, bandwidth):
    """float64 rows max(softmax(-D / (2 bw^2)), 2^-100) of D [Q,n]."""
    logits = -D.double() / (2.0 * float(bandwidth) ** 2)
    return torch.clamp_min(torch.softmax(logits, dim=1), FLOOR_W)


def _tiny_inputs():
    shape, seed, regime = W.cases.CASES[0]                     # ("tiny", 0, "near")
    return {k: torch.from_numpy(v).double() for k, v in W.cases.gen_inputs(shape, seed, regime).items()}


ARGS = ("h_fake", "m_real", "h_real", "m_fake")


def test_one_query_is_the_weighted_loss_exactly():
    inp = _tiny_inputs()
    B = inp["real"].shape[0]
    w0 = W.random_weights(B, 5)
    want, _, _ = W.weighted_loss(inp["real"], inp["fake"], W.cases.SC, 0.8, 30, *(inp[k] for k in ARGS), w0, w0)
    got = conditional_loss(inp["real"], inp["fake"], W.cases.SC, 0.8, 30, *(inp[k] for k in ARGS), w0[None])
    assert float(got) == float(want)
    got1 = conditional_loss(inp["real"], inp["fake"], W.cases.SC, 0.8, 30, *(inp[k] for k in ARGS), w0[None],
                            torch.ones(1, dtype=F64))
    assert float(got1) == float(want)


def test_loss_from_costs_agrees_with_the_loss_from_videos_and_is_linear_in_omega():
    inp = _tiny_inputs()
    B = inp["real"].shape[0]
    x, y = inp["real"].reshape(B, 1, -1), inp["fake"].reshape(B, 1, -1)
    C3 = torch.stack([W.ot.modified_cost(x, y, inp["h_fake"], inp["m_real"], W.cases.SC),
                      W.ot.modified_cost(x, x, inp["h_real"], inp["m_real"], W.cases.SC),
                      W.ot.modified_cost(y, y, inp["h_fake"], inp["m_fake"], W.cases.SC)])
    w = torch.stack([W.random_weights(B, 50 + q) for q in range(3)])
    omega = torch.tensor([0.5, 0.2, 0.3], dtype=F64)
    for om in (None, omega):
        a, costs, nits = conditional_loss_from_costs(C3, w, om, 0.8, 12)
        b = conditional_loss(inp["real"], inp["fake"], W.cases.SC, 0.8, 12, *(inp[k] for k in ARGS), w, om)
        assert abs(float(a) - float(b)) <= 1e-13 * max(1.0, abs(float(b)))
        assert nits == [[12] * 3] * 3
    per_q = [float(2.0 * c[0] - c[1] - c[2]) for c in costs]
    assert abs(float(a) - sum(o * p for o, p in zip(omega.tolist(), per_q))) <= 1e-13 * max(1.0, abs(float(a)))
    assert len({round(p, 9) for p in per_q}) == 3               # the weight rows matter


def test_weights_yardstick_uniform_at_a_huge_bandwidth_and_floored_at_a_tiny_one():
    g = torch.Generator().manual_seed(3)
    for Q, n in ((1, 1), (3, 5), (5, 67), (2, 1024)):
        c = torch.rand(n, 7, generator=g, dtype=F64)
        D = torch.cdist(c[:Q], c) ** 2
        w = conditional_weights(D, 1e30)
        assert bool((w == 1.0 / n).all())
        w = conditional_weights(D, 0.7)
        assert float((w.sum(1) - 1.0).abs().max()) <= 1e-14 and bool((w > 0).all())
        if n > 1:
            w = conditional_weights(D, 1e-3)                    # off-diagonal terms underflow: the floor, exactly
            off = torch.ones(Q, n, dtype=torch.bool)
            off[torch.arange(Q), torch.arange(Q)] = False
            assert bool((w[off] == FLOOR_W).all()) and bool((w[~off] == 1.0).all())
    assert np.float32(FLOOR_W) == FLOOR_W and np.log2(np.float32(FLOOR_W)) == -100.0     # a normal fp32 number, exact log2


# ================================================================ header, ctypes table, argument validation
def _decls():
    text = open(os.path.join(ROOT, "include", "kccot_conditional.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_is_strict_c99_and_matches_the_ctypes_table(tmp_path):
    from kccotgan_amd import _lib
    decls = _decls()
    assert len(decls) == 7
    assert sorted(decls) == sorted(_lib.CONDITIONAL_SIGNATURES), "ctypes table and header disagree"
    others = (set(_lib.SIGNATURES) | set(_lib.MODEL_SIGNATURES) | set(_lib.WEIGHTED_SIGNATURES) | set(_lib.SMOOTH3C_SIGNATURES))
    assert not set(_lib.CONDITIONAL_SIGNATURES) & others
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "unsigned": ctypes.c_uint,
             "size_t": ctypes.c_size_t}
    for name, args in decls.items():
        assert hasattr(_lib.lib, name), "libkccot.so does not export %s" % name
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        assert _lib.CONDITIONAL_SIGNATURES[name][1] == want, name
        assert getattr(_lib.lib, name).argtypes == want
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_conditional.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(probe), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_happens_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is rejected on its arguments
    EINVAL, EWORKSPACE, EUNSUPPORTED = _lib.EINVAL, _lib.EWORKSPACE, _lib.EUNSUPPORTED

    def wts(D=one, Q=2, n=8, bw=1.0, out=one):
        return lib.kccot_conditional_weights_f32(D, Q, n, bw, out, None)

    assert wts(D=None) == EINVAL and wts(out=None) == EINVAL and wts(Q=0) == EINVAL and wts(n=0) == EINVAL
    assert wts(bw=0.0) == EINVAL and wts(bw=-1.0) == EINVAL and wts(bw=float("nan")) == EINVAL
    assert b"bandwidth" in lib.kccot_last_error()
    assert wts(n=1025) == EUNSUPPORTED

    need8, need130 = lib.kccot_sinkhorn_conditional_workspace_bytes(2, 8), lib.kccot_sinkhorn_conditional_workspace_bytes(2, 130)
    assert 0 < need8 < need130 and need8 % 4 == 0 and need130 % 4 == 0
    assert lib.kccot_sinkhorn_conditional_workspace_bytes(0, 8) == 0 and lib.kccot_sinkhorn_conditional_workspace_bytes(2, 1025) == 0
    # the 3 Q per-problem gradients, and above n = 128 ONE transposed copy of C3 (not Q) beside the 3 Q column accumulators
    assert need8 >= 3 * 2 * 8 * 8 * 4 and need130 >= (3 * 2 + 3 + 3 * 2) * 130 * 130 * 4
    assert need130 < (3 * 2 + 3 * 2 + 3 * 2) * 130 * 130 * 4

    def fwd(C3=one, w=one, Q=2, n=8, eps=1.0, L=10, uh=None, vh=None, cost=one, nits=one, loss=one, ws=one, wsb=need8):
        return lib.kccot_sinkhorn_conditional_fwd_f32(C3, w, None, Q, n, eps, L, 10, 0.01, uh, vh, cost, nits, loss, ws, wsb, None)

    def bwd(g=one, C3=one, w=one, uh=one, vh=one, nits=one, Q=2, n=8, eps=1.0, L=10, dC=one, ws=one, wsb=need8):
        return lib.kccot_sinkhorn_conditional_bwd_f32(g, C3, w, None, uh, vh, nits, Q, n, eps, L, dC, ws, wsb, None)

    for f in (fwd, bwd):
        assert f(C3=None) == EINVAL and f(w=None) == EINVAL and f(nits=None) == EINVAL
        assert f(Q=0) == EINVAL and f(n=0) == EINVAL and f(eps=0.0) == EINVAL and f(eps=-1.0) == EINVAL and f(L=-1) == EINVAL
        assert f(n=1025) == EUNSUPPORTED
        assert f(wsb=need8 - 1) == EWORKSPACE and f(ws=None) == EWORKSPACE
        assert f(n=130, wsb=need130 - 1) == EWORKSPACE
    assert fwd(cost=None) == EINVAL and fwd(loss=None) == EINVAL
    assert fwd(uh=one) == EINVAL and fwd(vh=one) == EINVAL
    assert b"together" in lib.kccot_last_error()
    assert bwd(g=None) == EINVAL and bwd(uh=None) == EINVAL and bwd(vh=None) == EINVAL and bwd(dC=None) == EINVAL

    B, K, Q = 8, 64, 3
    lneed = lib.kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, Q)
    assert lneed >= 3 * B * B * 4 + lib.kccot_sinkhorn_conditional_workspace_bytes(Q, B)
    assert lneed >= lib.kccot_pairwise_cost3_workspace_bytes(B, K) and lneed >= lib.kccot_pairwise_cost3_bwd_workspace_bytes(B, K)
    assert lib.kccot_conditional_sinkhorn_loss_workspace_bytes(0, K, Q) == 0
    assert lib.kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, 0) == 0

    def lfwd(real=one, w=one, B=B, Q=Q, T=4, eps=1.0, L=10, C3=one, uh=None, vh=None, flags=0, wsb=lneed):
        return lib.kccot_conditional_sinkhorn_loss_fwd_f32(real, one, B, K, 1.0, one, one, one, one, T, 3, eps, L, 10, 0.01, flags,
                                                           w, None, Q, C3, uh, vh, one, one, one, one, wsb, None)

    def lbwd(real=one, w=one, B=B, Q=Q, T=4, eps=1.0, L=10, C3=one, wsb=lneed):
        return lib.kccot_conditional_sinkhorn_loss_bwd_f32(one, real, one, B, K, 1.0, one, one, one, one, T, 3, eps, L, w, None, Q,
                                                           C3, one, one, one, one, None, None, None, None, one, wsb, None)

    for f in (lfwd, lbwd):
        assert f(real=None) == EINVAL and f(w=None) == EINVAL and f(C3=None) == EINVAL
        assert f(B=0) == EINVAL and f(Q=0) == EINVAL and f(T=0) == EINVAL and f(eps=0.0) == EINVAL and f(L=-1) == EINVAL
        assert f(B=1025, wsb=1 << 40) == EUNSUPPORTED
        assert f(wsb=lneed - 1) == EWORKSPACE
    assert lfwd(uh=one) == EINVAL and lfwd(flags=_lib.COST_RBF_SUM) == EINVAL


def test_python_wrappers_are_exported_and_refuse_what_they_cannot_do():
    import inspect
    from kccotgan_amd import gan_utils as g, _lib
    assert "kernel_conditional_weights" in g.__all__ and "compute_conditional_sinkhorn_loss" in g.__all__
    assert list(inspect.signature(g.kernel_conditional_weights).parameters) == ["context", "bandwidth", "queries"]
    p = inspect.signature(g.compute_conditional_sinkhorn_loss).parameters
    assert list(p) == ["f_real", "f_fake", "scaling_coef", "sinkhorn_eps", "sinkhorn_l", "h_fake", "m_real", "h_real", "m_fake",
                       "weights", "query_weights", "video"]
    assert p["query_weights"].default is None and p["video"].default is True
    x, f, w = torch.zeros(2, 3, 4), torch.zeros(2, 3, 2), torch.full((3, 2), 0.5)
    # none of these touches a device: the refusal comes first
    with pytest.raises(NotImplementedError):
        g.kernel_conditional_weights(x.clone().requires_grad_(True), 1.0)
    for bw in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            g.kernel_conditional_weights(x, bw)
    with pytest.raises(NotImplementedError):
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w.clone().requires_grad_(True), video=False)
    with pytest.raises(NotImplementedError):
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w, torch.ones(3).requires_grad_(True), video=False)
    with pytest.raises(NotImplementedError):
        g.compute_conditional_sinkhorn_loss(x.clone().requires_grad_(True), x, 1.0, 1.0, 10, f, f, f, f, w, video=False)
    with pytest.raises(ValueError):
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, torch.full((2,), 0.5), video=False)
    with pytest.raises(ValueError):
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w, torch.ones(4), video=False)
    with pytest.raises(_lib.KccotError):                       # well-formed, but there is no CPU path
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w, video=False)
    with pytest.raises(_lib.KccotError):
        g.kernel_conditional_weights(x, 1.0)


def test_trainer_option_conflicts_are_refused_before_anything_is_built():
    from kccotgan_amd.kernel_train import KCCOTTrainer
    with pytest.raises(ValueError, match="conditional_bandwidth"):
        KCCOTTrainer(2, device="cpu", conditional_bandwidth=0.2, mixed_sinkhorn=True)
    with pytest.raises(ValueError, match="conditional_bandwidth"):
        KCCOTTrainer(2, device="cpu", conditional_bandwidth=0.2, bi_causal=True)
    with pytest.raises(NotImplementedError, match="sharded"):
        KCCOTTrainer(2, device="cpu", conditional_bandwidth=0.2, group=object())
    with pytest.raises(ValueError):
        KCCOTTrainer(2, device="cpu", conditional_bandwidth=0.0)
