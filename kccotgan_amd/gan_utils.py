"""Drop-in for the reference's ``gan_utils.py`` -- same function names, argument order, defaults
and positional behaviour -- with ``torch.Tensor`` on a ROCm device instead of ``tf.Tensor`` and
the arithmetic done by the hand-written HIP kernels behind ``include/kccot.h``.

Every function cites the reference lines it replaces (``gan_utils.py:LINE`` = /root/reference).
Differentiable with hand-written backward kernels (the reference differentiates through the
unrolled Sinkhorn loop with tf.GradientTape, kernel_train.py:221,252,262,289).

There is no CPU path: tensors must live on the GPU and the library must be built.
"""
import collections

import torch

from . import _lib
from ._lib import lib, check, ptr, stream_of, workspace

__all__ = ["cost_xy", "modified_cost", "bi_causal_modified_cost", "benchmark_sinkhorn",
           "compute_sinkhorn", "compute_N", "scale_invariante_martingale_regularization",
           "compute_sinkhorn_loss", "compute_mixed_sinkhorn_loss", "compute_bicausal_sinkhorn_loss",
           "compute_weighted_sinkhorn", "compute_weighted_sinkhorn_loss", "kernel_conditional_weights",
           "compute_conditional_sinkhorn_loss", "compute_kernel_conditional_sinkhorn_loss", "last_info",
           "raise_if_solver_aborted"]

# executed Sinkhorn iteration counts (device int32 tensors, no host sync) of the latest calls;
# the reference keeps them in a local (gan_utils.py:148,158) although its docstring promises them
last_info = {}

# cost-kernel selection for tests/bench: 0 = automatic, or _lib.COST_FORCE_DIRECT / _lib.COST_FORCE_MFMA
cost_flags = 0

_THRESH = 10 ** (-2)   # gan_utils.py:91,144
_LMIN = 100            # gan_utils.py:149


def _flat2(x):
    """[B, ...] -> contiguous fp32 [B, K].  cost_xy sums over ALL trailing axes
    (gan_utils.py:16-17), so any trailing shape -- including the un-transposed [B,H,T,W,C]
    video (gan_utils.py:217-220) -- is just a row of K numbers."""
    if x.dim() < 2:
        raise ValueError("expected [batch, ...], got shape %s" % (tuple(x.shape),))
    _lib.require_gpu(x)
    x = x.reshape(x.shape[0], -1)
    if x.dtype != torch.float32:
        x = x.float()
    return x.contiguous()


def _gpu_f32(t):
    """A device tensor as contiguous fp32 (None stays None)."""
    if t is None:
        return None
    _lib.require_gpu(t)
    return (t if t.dtype == torch.float32 else t.float()).contiguous()


def _feat(t):
    if t.dim() != 3:
        raise ValueError("h / M must be [batch, time steps, J], got %s" % (tuple(t.shape),))
    return _gpu_f32(t)


def _same(x, y):
    return x.data_ptr() == y.data_ptr() and x.shape == y.shape


def _pairwise_forward(ctx, x, y, h1, M1, h2, M2, sc, flags):
    """The forward of _PairwiseCost and _PairwiseCostL1: kccot_pairwise_cost_f32 with `flags` (and COST_SAME when x is y)"""
    Bx, K = x.shape
    By = y.shape[0]
    if y.shape[1] != K:
        raise ValueError("x and y disagree on the feature count: %d vs %d" % (K, y.shape[1]))
    T = J = 1
    for h, M in ((h1, M1), (h2, M2)):
        if h is not None:
            if h.shape[0] != Bx or M.shape[0] != By or h.shape[1:] != M.shape[1:]:
                raise ValueError("h must be [Bx,T,J] and M [By,T,J]; got %s and %s"
                                 % (tuple(h.shape), tuple(M.shape)))
            T, J = h.shape[1], h.shape[2]
    same = _same(x, y)
    flags = (_lib.COST_SAME if same else 0) | flags
    C = _lib.empty((Bx, By), torch.float32, x.device)
    ws, wsb = workspace(lib.kccot_pairwise_cost_workspace_bytes(Bx, By, K), x)
    check(lib.kccot_pairwise_cost_f32(ptr(x), ptr(y), Bx, By, K, sc, ptr(h1), ptr(M1), ptr(h2), ptr(M2),
                                      T, J, flags, ptr(C), ws, wsb, stream_of(x)), "pairwise_cost")
    ctx.save_for_backward(x, y, h1, M1, h2, M2)
    ctx.sc, ctx.same, ctx.TJ = sc, same, (T, J)
    return C


class _PairwiseCost(torch.autograd.Function):
    """C = cost_xy(x, y) [+ causal(h1, M1)] [+ causal(h2, M2)]   (gan_utils.py:6-72)"""

    @staticmethod
    def forward(ctx, x, y, h1, M1, h2, M2, sc):
        return _pairwise_forward(ctx, x, y, h1, M1, h2, M2, sc, cost_flags)

    @staticmethod
    def backward(ctx, g):
        x, y, h1, M1, h2, M2 = ctx.saved_tensors
        g = g.contiguous()
        Bx, K = x.shape
        By = y.shape[0]
        T, J = ctx.TJ
        need = ctx.needs_input_grad
        want_x, want_y = need[0], need[1] and not ctx.same
        if ctx.same:
            want_x = need[0] or need[1]
        dx = _lib.empty_like(x) if want_x else None
        dy = _lib.empty_like(y) if want_y else None
        dh1 = _lib.empty_like(h1) if (h1 is not None and need[2]) else None
        dM1 = _lib.empty_like(M1) if (M1 is not None and need[3]) else None
        dh2 = _lib.empty_like(h2) if (h2 is not None and need[4]) else None
        dM2 = _lib.empty_like(M2) if (M2 is not None and need[5]) else None
        flags = _lib.COST_SAME if ctx.same else 0
        ws, wsb = workspace(lib.kccot_pairwise_cost_bwd_workspace_bytes(Bx, By), x)
        st = stream_of(x)
        if dx is not None or dy is not None or dh1 is not None or dM1 is not None:
            check(lib.kccot_pairwise_cost_bwd_f32(ptr(g), ptr(x), ptr(y), Bx, By, K, ctx.sc, ptr(h1), ptr(M1), T, J,
                                                  flags, ptr(dx), ptr(dy), ptr(dh1), ptr(dM1), ws, wsb, st),
                  "pairwise_cost_bwd")
        if dh2 is not None or dM2 is not None:
            check(lib.kccot_pairwise_cost_bwd_f32(ptr(g), ptr(x), ptr(y), Bx, By, K, ctx.sc, ptr(h2), ptr(M2), T, J,
                                                  flags, None, None, ptr(dh2), ptr(dM2), ws, wsb, st),
                  "pairwise_cost_bwd")
        if ctx.same:
            # x and y are one tensor: its whole gradient is returned once (autograd would add the two)
            return (dx if need[0] else None), (dx if (need[1] and not need[0]) else None), dh1, dM1, dh2, dM2, None
        return dx, dy, dh1, dM1, dh2, dM2, None


def _cost3_forward(ctx, real, fake, h_fake, h_real, m_real, m_fake, sc, flags):
    """The forward of _Cost3 and _Cost3L1: kccot_pairwise_cost3_f32 with `flags`"""
    B, K = real.shape
    if fake.shape != real.shape:
        raise ValueError("real and fake must have the same shape: %s vs %s" % (tuple(real.shape), tuple(fake.shape)))
    T, J = h_fake.shape[1], h_fake.shape[2]
    for t in (h_fake, h_real, m_real, m_fake):
        if tuple(t.shape) != (B, T, J):
            raise ValueError("h / M must all be [%d,%d,%d]; got %s" % (B, T, J, tuple(t.shape)))
    C3 = _lib.empty((3, B, B), torch.float32, real.device)
    ws, wsb = workspace(lib.kccot_pairwise_cost3_workspace_bytes(B, K), real)
    check(lib.kccot_pairwise_cost3_f32(ptr(real), ptr(fake), B, K, sc, ptr(h_fake), ptr(h_real), ptr(m_real),
                                       ptr(m_fake), T, J, flags, ptr(C3), ws, wsb, stream_of(real)),
          "pairwise_cost3")
    ctx.save_for_backward(real, fake, h_fake, h_real, m_real, m_fake)
    ctx.sc = sc
    return C3


class _Cost3(torch.autograd.Function):
    """The three cost matrices of compute_sinkhorn_loss (gan_utils.py:221-223), one pass over the videos."""

    @staticmethod
    def forward(ctx, real, fake, h_fake, h_real, m_real, m_fake, sc):
        return _cost3_forward(ctx, real, fake, h_fake, h_real, m_real, m_fake, sc, cost_flags)

    @staticmethod
    def backward(ctx, g3):
        real, fake, h_fake, h_real, m_real, m_fake = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289); "
                                      "use compute_sinkhorn for a gradient w.r.t. both operands")
        g3 = g3.contiguous()
        B, K = real.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        need = ctx.needs_input_grad
        dfake = _lib.empty_like(fake) if need[1] else None
        dhf = _lib.empty_like(h_fake) if need[2] else None
        dhr = _lib.empty_like(h_real) if need[3] else None
        dmr = _lib.empty_like(m_real) if need[4] else None
        dmf = _lib.empty_like(m_fake) if need[5] else None
        ws, wsb = workspace(lib.kccot_pairwise_cost3_bwd_workspace_bytes(B, K), real)
        check(lib.kccot_pairwise_cost3_bwd_f32(ptr(g3), ptr(real), ptr(fake), B, K, ctx.sc, ptr(h_fake), ptr(h_real),
                                               ptr(m_real), ptr(m_fake), T, J, ptr(dfake), ptr(dhf), ptr(dhr),
                                               ptr(dmr), ptr(dmf), ws, wsb, stream_of(real)), "pairwise_cost3_bwd")
        return None, dfake, dhf, dhr, dmr, dmf, None


class _PairwiseCostL1(torch.autograd.Function):
    """_PairwiseCost with the L1 ground cost sc * sum_k |x[i,k] - y[j,k]| (COST_L1; an extension: the reference's docstrings
    name this cost, its code squares).  The forward is the direct-difference kernel; the video gradients come from
    kccot_l1_cost_bwd_f32 (include/kccot_l1.h), the feature gradients -- which do not depend on the ground cost -- from the
    squared cost's backward called without video outputs."""

    @staticmethod
    def forward(ctx, x, y, h1, M1, h2, M2, sc):
        return _pairwise_forward(ctx, x, y, h1, M1, h2, M2, sc, _lib.COST_L1)

    @staticmethod
    def backward(ctx, g):
        x, y, h1, M1, h2, M2 = ctx.saved_tensors
        g = g.contiguous()
        Bx, K = x.shape
        By = y.shape[0]
        T, J = ctx.TJ
        need = ctx.needs_input_grad
        want_x = (need[0] or need[1]) if ctx.same else need[0]
        want_y = need[1] and not ctx.same
        dx = _lib.empty_like(x) if want_x else None
        dy = _lib.empty_like(y) if want_y else None
        flags = _lib.COST_SAME if ctx.same else 0
        st = stream_of(x)
        if dx is not None or dy is not None:
            ws, wsb = workspace(lib.kccot_l1_cost_bwd_workspace_bytes(Bx, By), x)
            check(lib.kccot_l1_cost_bwd_f32(ptr(g), ptr(x), ptr(y), Bx, By, K, ctx.sc, flags, ptr(dx), ptr(dy), ws, wsb, st),
                  "l1_cost_bwd")
        grads = []
        for k, (h, M) in enumerate(((h1, M1), (h2, M2))):
            dh = _lib.empty_like(h) if (h is not None and need[2 + 2 * k]) else None
            dM = _lib.empty_like(M) if (M is not None and need[3 + 2 * k]) else None
            if dh is not None or dM is not None:
                check(lib.kccot_pairwise_cost_bwd_f32(ptr(g), ptr(x), ptr(y), Bx, By, K, ctx.sc, ptr(h), ptr(M), T, J, flags,
                                                      None, None, ptr(dh), ptr(dM), None, 0, st), "pairwise_cost_bwd")
            grads += [dh, dM]
        if ctx.same:
            # x and y are one tensor: its whole gradient is returned once (autograd would add the two)
            return ((dx if need[0] else None), (dx if (need[1] and not need[0]) else None), *grads, None)
        return (dx, dy, *grads, None)


class _Cost3L1(torch.autograd.Function):
    """_Cost3 with the L1 ground cost (COST_L1): one pass of the direct-difference kernel over the three problems; dfake from
    kccot_l1_cost3_bwd_f32, the feature gradients from kccot_pairwise_cost3_bwd_f32 with dfake = NULL."""

    @staticmethod
    def forward(ctx, real, fake, h_fake, h_real, m_real, m_fake, sc):
        return _cost3_forward(ctx, real, fake, h_fake, h_real, m_real, m_fake, sc, _lib.COST_L1)

    @staticmethod
    def backward(ctx, g3):
        real, fake, h_fake, h_real, m_real, m_fake = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289); "
                                      "use compute_sinkhorn for a gradient w.r.t. both operands")
        g3 = g3.contiguous()
        B, K = real.shape
        T, J = h_fake.shape[1], h_fake.shape[2]
        need = ctx.needs_input_grad
        st = stream_of(real)
        dfake = _lib.empty_like(fake) if need[1] else None
        if dfake is not None:
            ws, wsb = workspace(lib.kccot_l1_cost3_bwd_workspace_bytes(B), real)
            check(lib.kccot_l1_cost3_bwd_f32(ptr(g3), ptr(real), ptr(fake), B, K, ctx.sc, ptr(dfake), ws, wsb, st), "l1_cost3_bwd")
        dhf = _lib.empty_like(h_fake) if need[2] else None
        dhr = _lib.empty_like(h_real) if need[3] else None
        dmr = _lib.empty_like(m_real) if need[4] else None
        dmf = _lib.empty_like(m_fake) if need[5] else None
        if any(d is not None for d in (dhf, dhr, dmr, dmf)):      # (no video output: no workspace)
            check(lib.kccot_pairwise_cost3_bwd_f32(ptr(g3), ptr(real), ptr(fake), B, K, ctx.sc, ptr(h_fake), ptr(h_real),
                                                   ptr(m_real), ptr(m_fake), T, J, None, ptr(dhf), ptr(dhr), ptr(dmr),
                                                   ptr(dmf), None, 0, st), "pairwise_cost3_bwd")
        return None, dfake, dhf, dhr, dmr, dmf, None


def _ground(ground_cost):
    """True for the L1 ground cost, False for the squared one (the reference's code and the default)."""
    if ground_cost not in ("l1", "l2"):
        raise ValueError("ground_cost must be 'l2' (squared distance, the reference's code) or 'l1'; got %r" % (ground_cost,))
    return ground_cost == "l1"


class _Sinkhorn(torch.autograd.Function):
    """cost[p] = sum(pi_p * C_p) after the Sinkhorn loop on C [nprob,n,n] (gan_utils.py:138-165)."""

    @staticmethod
    def forward(ctx, C, eps, L, Lmin, stop_mode, tag):
        nprob, n, _ = C.shape
        C = C.contiguous()
        dev = C.device
        keep = ctx.needs_input_grad[0]
        Lh = max(int(L), 1)
        u_hist = _lib.empty((nprob, Lh, n), torch.float32, dev) if keep else None
        v_hist = _lib.empty((nprob, Lh, n), torch.float32, dev) if keep else None
        cost = _lib.empty((nprob,), torch.float32, dev)
        nits = _lib.empty((2 * nprob,), torch.int32, dev)   # [reference-equivalent counts | iterations executed]
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(nprob, n), C)
        check(lib.kccot_sinkhorn_fwd_f32(ptr(C), nprob, n, float(eps), int(L), int(Lmin), _THRESH, stop_mode,
                                         ptr(u_hist), ptr(v_hist), ptr(cost), ptr(nits), None, ws, wsb,
                                         stream_of(C)), "sinkhorn_fwd")
        last_info[tag], last_info[tag + "_executed"] = nits[:nprob], nits[nprob:]
        if keep:
            ctx.save_for_backward(C, u_hist, v_hist, nits)
        ctx.eps, ctx.Lh = float(eps), Lh
        return cost

    @staticmethod
    def backward(ctx, gcost):
        C, u_hist, v_hist, nits = ctx.saved_tensors
        nprob, n, _ = C.shape
        gcost = gcost.contiguous().float()
        dC = _lib.empty_like(C)
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(nprob, n), C)
        check(lib.kccot_sinkhorn_bwd_f32(ptr(C), ptr(u_hist), ptr(v_hist), ptr(nits), nprob, n, ctx.eps, ctx.Lh,
                                         ptr(gcost), ptr(dC), ws, wsb, stream_of(C)), "sinkhorn_bwd")
        return dC, None, None, None, None, None


_tickets = {}


def _ticket(device):
    """One zero-initialised device int per device: the arrival counter of the fused divergence kernel
    (the kernel leaves it at zero)."""
    t = _tickets.get(device)
    if t is None:
        t = torch.zeros((1,), dtype=torch.int32, device=device)
        _tickets[device] = t
    return t


def _divergence_fwd(C3, eps, L, Lmin):
    """The three solves of C3 [3,n,n] AND 2 xy - xx - yy (gan_utils.py:221-225): one launch at n <= 128, two inside the
    library above.  Returns (cost3 | loss, nits, what _divergence_bwd needs)."""
    _, n, _ = C3.shape
    dev = C3.device
    Lh = max(int(L), 1)
    u_hist = _lib.empty((3, Lh, n), torch.float32, dev)
    v_hist = _lib.empty((3, Lh, n), torch.float32, dev)
    small = _lib.empty((4,), torch.float32, dev)                                     # cost3 | loss
    nits = _lib.empty((6,), torch.int32, dev)           # [reference-equivalent counts | iterations executed]
    ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(3, n), C3)
    check(lib.kccot_sinkhorn_divergence_fwd_f32(ptr(C3), n, float(eps), int(L), int(Lmin), _THRESH, ptr(u_hist),
                                                ptr(v_hist), ptr(small), ptr(nits), ptr(small[3:]), ptr(_ticket(dev)),
                                                ws, wsb, stream_of(C3)), "sinkhorn_divergence_fwd")
    return small, nits, (C3, u_hist, v_hist, nits, float(eps), Lh)


def _divergence_bwd(saved, g):
    """d loss / d C3 scaled by the upstream scalar g, from what _divergence_fwd saved."""
    C3, u_hist, v_hist, nits, eps, Lh = saved
    _, n, _ = C3.shape
    g = g.reshape(1).contiguous().float()
    dC3 = _lib.empty_like(C3)
    ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(3, n), C3)
    if n > 128:   # streaming / cooperative solvers: weights first, then the generic reverse sweep
        gc = _lib.empty((3,), torch.float32, g.device)
        check(lib.kccot_mixed_divergence_bwd_f32(ptr(g), ptr(gc), stream_of(g)), "mixed_divergence_bwd")
        check(lib.kccot_sinkhorn_bwd_f32(ptr(C3), ptr(u_hist), ptr(v_hist), ptr(nits), 3, n, eps, Lh, ptr(gc), ptr(dC3),
                                         ws, wsb, stream_of(C3)), "sinkhorn_bwd")
    else:
        check(lib.kccot_sinkhorn_divergence_bwd_f32(ptr(C3), ptr(u_hist), ptr(v_hist), ptr(nits), n, eps, Lh, ptr(g),
                                                    ptr(dC3), ws, wsb, stream_of(C3)), "sinkhorn_divergence_bwd")
    return dC3


class _SinkhornDivergence(torch.autograd.Function):
    """loss = 2 W(C3[0]) - W(C3[1]) - W(C3[2]) in one launch each way (gan_utils.py:221-225)."""

    @staticmethod
    def forward(ctx, C3, eps, L, Lmin, tag):
        small, nits, saved = _divergence_fwd(C3.contiguous(), eps, L, Lmin)
        last_info[tag], last_info[tag + "_executed"] = nits[:3], nits[3:]
        last_info[tag + "_costs"] = small[:3]
        ctx.save_for_backward(*saved[:4])
        ctx.eps, ctx.Lh = saved[4:]
        return small[3:].reshape(())

    @staticmethod
    def backward(ctx, g):
        return _divergence_bwd((*ctx.saved_tensors, ctx.eps, ctx.Lh), g), None, None, None, None


def _pad64(n):
    return (n + 63) & ~63


def _weighted_path(n):
    """The solver a weighted solve of size n runs on (include/kccot_weighted.h): never the multi-CU solver, never the
    one-launch fused loss."""
    return "register" if n <= 128 else "streaming"


def _weights(w, n, name, normalize):
    """A weight vector as contiguous fp32 [n] on the device; ``normalize`` divides by its sum there (no host sync).  Plain
    torch operations: a gradient w.r.t. the returned vector reaches ``w`` through them."""
    if not torch.is_tensor(w):
        raise TypeError("%s must be a tensor of %d weights" % (name, n))
    _lib.require_gpu(w)
    if w.dim() != 1 or w.shape[0] != n:
        raise ValueError("%s must be [%d], got %s" % (name, n, tuple(w.shape)))
    w = w if w.dtype == torch.float32 else w.float()
    if normalize:
        w = w / w.sum()
    return w.contiguous()


class _WeightedSinkhorn(torch.autograd.Function):
    """_Sinkhorn with marginals a, b [nprob,n] (kccot_sinkhorn_weighted_fwd_f32 / _bwd_f32); when a or b wants a gradient the
    backward is kccot_sinkhorn_weighted_bwd_dw_f32 (include/kccot_weight_grad.h: the same dC bits, plus da, db)."""

    @staticmethod
    def forward(ctx, C, a, b, eps, L, Lmin, stop_mode, tag):
        nprob, n, _ = C.shape
        C = C.contiguous()
        dev = C.device
        keep = any(ctx.needs_input_grad[:3])
        Lh = max(int(L), 1)
        u_hist = _lib.empty((nprob, Lh, n), torch.float32, dev) if keep else None
        v_hist = _lib.empty((nprob, Lh, n), torch.float32, dev) if keep else None
        cost = _lib.empty((nprob,), torch.float32, dev)
        nits = _lib.empty((2 * nprob,), torch.int32, dev)   # [reference-equivalent counts | iterations executed]
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(nprob, n), C)
        check(lib.kccot_sinkhorn_weighted_fwd_f32(ptr(C), ptr(a), ptr(b), nprob, n, float(eps), int(L), int(Lmin), _THRESH,
                                                  stop_mode, ptr(u_hist), ptr(v_hist), ptr(cost), ptr(nits), None, ws, wsb,
                                                  stream_of(C)), "sinkhorn_weighted_fwd")
        last_info[tag], last_info[tag + "_executed"] = nits[:nprob], nits[nprob:]
        last_info[tag + "_path"] = _weighted_path(n)
        if keep:
            ctx.save_for_backward(C, a, b, u_hist, v_hist, nits)
        ctx.eps, ctx.Lh = float(eps), Lh
        return cost

    @staticmethod
    def backward(ctx, gcost):
        C, a, b, u_hist, v_hist, nits = ctx.saved_tensors
        nprob, n, _ = C.shape
        gcost = gcost.contiguous().float()
        dC = _lib.empty_like(C)
        ws, wsb = workspace(lib.kccot_sinkhorn_workspace_bytes(nprob, n), C)
        need = ctx.needs_input_grad
        if need[1] or need[2]:
            dab = _lib.empty((2, nprob, n), torch.float32, C.device)
            check(lib.kccot_sinkhorn_weighted_bwd_dw_f32(ptr(C), ptr(a), ptr(b), ptr(u_hist), ptr(v_hist), ptr(nits), nprob, n,
                                                         ctx.eps, ctx.Lh, ptr(gcost), ptr(dC), ptr(dab[0]), ptr(dab[1]), ws,
                                                         wsb, stream_of(C)), "sinkhorn_weighted_bwd_dw")
            return (dC if need[0] else None, dab[0] if need[1] else None, dab[1] if need[2] else None, None, None, None,
                    None, None)
        check(lib.kccot_sinkhorn_weighted_bwd_f32(ptr(C), ptr(a), ptr(b), ptr(u_hist), ptr(v_hist), ptr(nits), nprob, n,
                                                  ctx.eps, ctx.Lh, ptr(gcost), ptr(dC), ws, wsb, stream_of(C)),
              "sinkhorn_weighted_bwd")
        return dC, None, None, None, None, None, None, None


# What differs between the five losses _SinkhornLoss drives.  The entry points are called with the pointer arguments it
# assembles (w: the weight arguments, () for uniform marginals):
#   fwd(head, w, C, u_hist, v_hist, dC_unit, tail)
#       head = (real, fake, B, K, sc, *features, T, J, eps, L, Lmin, thresh, flags)
#       tail = (costs, nits, loss, [ticket,] ws, ws_bytes, stream)
#   bwd(gloss, inputs, hist, w, saved, dC_unit, outs, dw, tail)
#       inputs = (real, fake, B, K, sc, *features, T, J), hist = (eps, L), saved = (C, u_hist, v_hist, nits),
#       outs = (dfake, *dfeatures), dw = the weight-gradient arguments (() unless a weight wants one),
#       tail = (ws, ws_bytes, stream)
# The fused path (solves + reverse sweep in one launch; ``fusable``) passes dC_unit and null history, the history path the
# reverse.
#   P cost matrices, ``stack`` videos per operand ([x; x'] for the mixed loss), key: the last_info name of the matrices
#   real_hint: what the refusal of a gradient w.r.t. real points to;  ticket: the forward takes the arrival counter
#   queries: wa is [Q,B], one set of P solves per row (costs and counts are recorded as [Q,P]), and Q follows B, K in the
#            workspace queries ws_bytes (forward and plain backward) / dw_ws_bytes (weight-gradient backward)
#   dw(wa, small, want) -> (the dw arguments, (d wa, d wb)), want = which of (wa, wb) asks for a gradient
_OPERANDS_HINT = "; use %s for a gradient w.r.t. both operands"
_LossSpec = collections.namedtuple(
    "_LossSpec", "ws_bytes fwd bwd P stack key shape_error real_hint fusable ticket queries dw_ws_bytes dw",
    defaults=(3, 1, "_C3", "real and fake must have the same shape: {} vs {}", _OPERANDS_HINT % "compute_sinkhorn", True,
              True, False, None, None))


def _one_fwd(head, w, C, uh, vh, dCu, tail):
    if dCu is not None:
        check(lib.kccot_sinkhorn_loss_fused_fwd_f32(*head, C, dCu, *tail), "sinkhorn_loss_fused_fwd")
    else:
        check(lib.kccot_sinkhorn_loss_fwd_f32(*head, C, uh, vh, *tail), "sinkhorn_loss_fwd")


def _one_bwd(g, inputs, hist, w, saved, dCu, outs, dw, tail):
    if dCu is not None:
        check(lib.kccot_sinkhorn_loss_fused_bwd_f32(g, dCu, *inputs, *outs, *tail), "sinkhorn_loss_fused_bwd")
    else:
        check(lib.kccot_sinkhorn_loss_bwd_f32(g, *inputs, *hist, *saved, *outs, *tail), "sinkhorn_loss_bwd")


def _entry_points(name, unit_slot):
    """(fwd, bwd) on kccot_<name>_fwd_f32 / _bwd_f32 / _bwd_dw_f32 (when a weight wants a gradient); unit_slot: they take
    dC_unit behind the history."""
    f, b = getattr(lib, "kccot_%s_fwd_f32" % name), getattr(lib, "kccot_%s_bwd_f32" % name)
    bdw = getattr(lib, "kccot_%s_bwd_dw_f32" % name, None)

    def fwd(head, w, C, uh, vh, dCu, tail):
        check(f(*head, *w, C, uh, vh, *((dCu,) if unit_slot else ()), *tail), name + "_fwd")

    def bwd(g, inputs, hist, w, saved, dCu, outs, dw, tail):
        if dw:
            check(bdw(g, *inputs, *hist, *w, *saved, *outs, *dw, *tail), name + "_bwd_dw")
        else:
            check(b(g, *inputs, *hist, *w, *saved, *((dCu,) if unit_slot else ()), *outs, *tail), name + "_bwd")
    return fwd, bwd


def _weighted_dw(wa, small, want):
    dw = _lib.empty((2, wa.shape[0]), torch.float32, wa.device)
    return (ptr(dw[0]), ptr(dw[1])), (dw[0] if want[0] else None, dw[1] if want[1] else None)


def _conditional_dw(w, small, want):     # small[:3 Q]: the costs of the forward, which d omega is made of
    dw = _lib.empty(tuple(w.shape), torch.float32, w.device)
    dom = _lib.empty((w.shape[0],), torch.float32, w.device) if want[1] else None
    return (ptr(small[:3 * w.shape[0]]), ptr(dw), ptr(dom)), (dw if want[0] else None, dom)


_ONE_BATCH = _LossSpec(lib.kccot_sinkhorn_loss_workspace_bytes, _one_fwd, _one_bwd)
_BICAUSAL = _LossSpec(lib.kccot_bicausal_sinkhorn_loss_workspace_bytes, *_entry_points("bicausal_sinkhorn_loss", True))
_MIXED = _LossSpec(lib.kccot_mixed_sinkhorn_loss_workspace_bytes, *_entry_points("mixed_sinkhorn_loss", True), P=4, stack=2,
                   key="_Cmix", shape_error="the four videos must have the same shape")
# weighted marginals: always the dual-history path (the fused launch is not weighted)
_WEIGHTED = _LossSpec(lib.kccot_weighted_sinkhorn_loss_workspace_bytes, *_entry_points("weighted_sinkhorn_loss", False),
                      real_hint=_OPERANDS_HINT % "compute_weighted_sinkhorn", fusable=False,
                      dw_ws_bytes=lib.kccot_weighted_sinkhorn_loss_dw_workspace_bytes, dw=_weighted_dw)
_CONDITIONAL = _LossSpec(lib.kccot_conditional_sinkhorn_loss_workspace_bytes,
                         *_entry_points("conditional_sinkhorn_loss", False), real_hint="", fusable=False, ticket=False,
                         queries=True, dw_ws_bytes=lib.kccot_conditional_sinkhorn_loss_dw_workspace_bytes, dw=_conditional_dw)

# Where _SinkhornLoss.apply takes its tensors: (spec, tag, sc, eps, L, Lmin, real, fake, *features, wa, wb).  The weight pair
# closes the list, behind the 4 or 6 features, so that backward's tuple keeps (7 x None, dfake, *dfeatures) in front: the
# partial-gradient tests of the bi-causal and the mixed loss read the loss node by these positions.
_REAL, _FAKE, _FEATS, _WEIGHTS = 6, 7, 8, -2


class _SinkhornLoss(torch.autograd.Function):
    """A Sinkhorn loss of ``spec`` (_ONE_BATCH, _BICAUSAL, _MIXED, _WEIGHTED or _CONDITIONAL) as ONE library call each way:
    the cost matrices, the solves + their combination, and back.  (wa, wb), the last two arguments: None for uniform
    marginals, (w_real, w_fake) [B] each for _WEIGHTED, (w [Q,B] weight rows, omega [Q] query weights or None = 1/Q) for
    _CONDITIONAL.
    When a gradient is wanted and the dual history fits the CU's LDS (kccot_sinkhorn_fused_eligible: configs[0],
    configs[1]) the solves and the reverse sweep of an unweighted loss are ONE launch: no history leaves the CU, the state
    kept for backward is d loss / d C at dLoss = 1 and backward is coefficient build + video gradient only.  Otherwise the
    dual history path; when wa or wb wants a gradient its backward is the _bwd_dw entry point
    (include/kccot_weight_grad.h: the other gradients are the same bits).  Same kernels as _Cost3 followed by
    _SinkhornDivergence for the one-batch loss, a third of the host work."""

    @staticmethod
    def forward(ctx, spec, tag, sc, eps, L, Lmin, real, fake, *feats_and_weights):
        *feats, wa, wb = feats_and_weights
        rows, K = real.shape
        B = rows // spec.stack
        if fake.shape != real.shape or rows % spec.stack:
            raise ValueError(spec.shape_error.format(tuple(real.shape), tuple(fake.shape)))
        T, J = feats[0].shape[1], feats[0].shape[2]
        for t in feats:
            if t.shape != (B, T, J):
                raise ValueError("h / M must all be [%d,%d,%d]; got %s" % (B, T, J, tuple(t.shape)))
        need = ctx.needs_input_grad
        if need[_REAL]:
            raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)"
                                      + spec.real_hint)
        P, dev = spec.P, real.device
        q = (wa.shape[0],) if spec.queries else ()
        NP = P * (q[0] if q else 1)                                                 # solves
        keep = any(need[_FAKE:])                                                    # fake, features or weights
        Lh = max(int(L), 1)
        nc, nh = _pad64(P * B * B), _pad64(NP * Lh * B)
        small = _lib.empty((NP + 1,), torch.float32, dev)                            # costs | loss
        nits = _lib.empty((2 * NP,), torch.int32, dev)      # [reference-equivalent counts | iterations executed]
        st = stream_of(real)
        ws, wsb = workspace(spec.ws_bytes(B, K, *q), real, st)
        fused = bool(spec.fusable and keep and lib.kccot_sinkhorn_fused_eligible(B, int(L)))
        if fused:
            state = _lib.empty((2 * nc,), torch.float32, dev)                        # C | dC at dLoss = 1
            uh = vh = None
            dCu = ptr(state[nc:])
        else:
            state = _lib.empty((nc + (2 * nh if keep else 0),), torch.float32, dev)  # C | u_hist | v_hist
            uh, vh = (ptr(state[nc:nc + nh]), ptr(state[nc + nh:])) if keep else (None, None)
            dCu = None
        loss = small[NP:]
        spec.fwd((ptr(real), ptr(fake), B, K, sc, *map(ptr, feats), T, J, float(eps), int(L), int(Lmin), _THRESH, cost_flags),
                 () if wa is None else (ptr(wa), ptr(wb), *q), ptr(state), uh, vh, dCu,
                 (ptr(small), ptr(nits), ptr(loss), *((ptr(_ticket(dev)),) if spec.ticket else ()), ws, wsb, st))
        per_query = (lambda t: t.view(q[0], P)) if q else (lambda t: t)
        last_info[tag], last_info[tag + "_executed"] = per_query(nits[:NP]), per_query(nits[NP:])
        last_info[tag + "_costs"] = per_query(small[:NP])
        last_info[tag + spec.key] = state[:P * B * B].view(P, B, B)
        last_info[tag + "_fused_sweep"] = fused
        if wa is not None:
            last_info[tag + "_path"] = _weighted_path(B)
        if keep:
            ctx.save_for_backward(real, fake, *feats, wa, wb, state, nits, small)
        ctx.spec, ctx.cfg = spec, (float(sc), float(eps), Lh, fused)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        real, fake, *feats, wa, wb, state, nits, small = ctx.saved_tensors
        spec, (sc, eps, Lh, fused) = ctx.spec, ctx.cfg
        P, nf = spec.P, len(feats)
        rows, K = real.shape
        B = rows // spec.stack
        T, J = feats[0].shape[1], feats[0].shape[2]
        q = (wa.shape[0],) if spec.queries else ()
        nc, nh = _pad64(P * B * B), _pad64(P * (q[0] if q else 1) * Lh * B)
        need = ctx.needs_input_grad
        g = g.reshape(1).contiguous().float()
        dfake = _lib.empty_like(fake) if need[_FAKE] else None
        df = _lib.empty((nf, B, T, J), torch.float32, real.device) if any(need[_FEATS:_WEIGHTS]) else None
        dfeats = [(df[i] if need[_FEATS + i] else None) for i in range(nf)]
        want = need[_WEIGHTS:]
        dw, dwab = spec.dw(wa, small, want) if any(want) else ((), (None, None))
        st = stream_of(real)
        ws, wsb = workspace((spec.dw_ws_bytes if dw else spec.ws_bytes)(B, K, *q), real, st)
        if fused:
            saved, dCu = (None, None, None, None), ptr(state[nc:])
        else:
            saved, dCu = (ptr(state), ptr(state[nc:nc + nh]), ptr(state[nc + nh:]), ptr(nits)), None
        spec.bwd(ptr(g), (ptr(real), ptr(fake), B, K, sc, *map(ptr, feats), T, J), (eps, Lh),
                 () if wa is None else (ptr(wa), ptr(wb), *q), saved, dCu, (ptr(dfake), *map(ptr, dfeats)), dw, (ws, wsb, st))
        return (None,) * _FAKE + (dfake, *dfeats, *dwab)


class _KernelWeights(torch.autograd.Function):
    """w = max(softmax(-D / (2 bw^2)), 2^-100) by rows (kccot_conditional_weights_f32) with its adjoint
    (kccot_conditional_weights_bwd_f32, include/kccot_weight_grad.h).  ``bw``: a Python float (a constant), or a 0-dim fp32
    device tensor, which is read on the device (the _dev entry points: no host read, the same bits) and differentiated."""

    @staticmethod
    def forward(ctx, D, bw):
        Q, B = D.shape
        w = _lib.empty((Q, B), torch.float32, D.device)
        if torch.is_tensor(bw):
            check(lib.kccot_conditional_weights_dev_f32(ptr(D), Q, B, ptr(bw), ptr(w), stream_of(D)), "conditional_weights")
        else:
            check(lib.kccot_conditional_weights_f32(ptr(D), Q, B, bw, ptr(w), stream_of(D)), "conditional_weights")
        ctx.save_for_backward(D, w, *([bw] if torch.is_tensor(bw) else []))
        ctx.bw = None if torch.is_tensor(bw) else bw
        return w

    @staticmethod
    def backward(ctx, dw):
        D, w, *bwt = ctx.saved_tensors
        Q, B = D.shape
        dw = dw.contiguous().float()
        dD = _lib.empty((Q, B), torch.float32, D.device)
        dbw = _lib.empty((Q,), torch.float32, D.device)
        if bwt:
            check(lib.kccot_conditional_weights_bwd_dev_f32(ptr(D), ptr(w), ptr(dw), Q, B, ptr(bwt[0]), ptr(dD), ptr(dbw),
                                                            stream_of(D)), "conditional_weights_bwd")
        else:
            check(lib.kccot_conditional_weights_bwd_f32(ptr(D), ptr(w), ptr(dw), Q, B, ctx.bw, ptr(dD), ptr(dbw),
                                                        stream_of(D)), "conditional_weights_bwd")
        gbw = dbw.double().sum().float().reshape(()) if (bwt and ctx.needs_input_grad[1]) else None   # the Q row terms
        return (dD if ctx.needs_input_grad[0] else None), gbw


class _MixedDivergence(torch.autograd.Function):
    """loss = 2*W_xy - W_xx - W_yy (gan_utils.py:225) as one launch each way."""

    @staticmethod
    def forward(ctx, cost3):
        loss = _lib.empty((1,), torch.float32, cost3.device)
        check(lib.kccot_mixed_divergence_fwd_f32(ptr(cost3), ptr(loss), stream_of(cost3)), "mixed_divergence_fwd")
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        g = g.reshape(1).contiguous().float()
        gc = _lib.empty((3,), torch.float32, g.device)
        check(lib.kccot_mixed_divergence_bwd_f32(ptr(g), ptr(gc), stream_of(g)), "mixed_divergence_bwd")
        return gc


class _Martingale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, lam, sc):
        B, T, J = M.shape
        pm = _lib.empty((1,), torch.float32, M.device)
        check(lib.kccot_martingale_fwd_f32(ptr(M), B, T, J, lam, sc, ptr(pm), stream_of(M)), "martingale_fwd")
        ctx.save_for_backward(M)
        ctx.lam, ctx.sc = lam, sc
        return pm.reshape(())

    @staticmethod
    def backward(ctx, g):
        (M,) = ctx.saved_tensors
        B, T, J = M.shape
        g = g.reshape(1).contiguous().float()
        dM = _lib.empty_like(M)
        check(lib.kccot_martingale_bwd_f32(ptr(M), B, T, J, ctx.lam, ctx.sc, ptr(g), ptr(dM), stream_of(M)),
              "martingale_bwd")
        return dM, None, None


# ------------------------------------------------------------------------------------------------
# the reference's public functions
# ------------------------------------------------------------------------------------------------
def cost_xy(x, y, scaling_coef, *, ground_cost="l2"):
    """gan_utils.py:6-18.  x, y: [batch, time steps, features] -> [batch_x, batch_y] matrix of
    scaling_coef * squared L2 distance summed over time and features.

    ``ground_cost="l1"`` (keyword-only, not in the reference, here and in the functions below): the sum of absolute
    differences the reference's docstrings describe instead of the squared distance its code computes."""
    return (_PairwiseCostL1 if _ground(ground_cost) else _PairwiseCost).apply(
        _flat2(x), _flat2(y), None, None, None, None, float(scaling_coef))


def modified_cost(x, y, h, M, scaling_coef, *, ground_cost="l2"):
    """gan_utils.py:21-43.  cost_xy + scaling_coef * sum_{t<T-1} h[i,t]*(M[j,t+1]-M[j,t]):
    h indexes rows, M indexes columns (gan_utils.py:37)."""
    return (_PairwiseCostL1 if _ground(ground_cost) else _PairwiseCost).apply(
        _flat2(x), _flat2(y), _feat(h), _feat(M), None, None, float(scaling_coef))


def bi_causal_modified_cost(x, y, hy, Mx, hx, My, scaling_coef, *, ground_cost="l2"):
    """gan_utils.py:46-72.  cost_xy + C_hM(hy, Mx) + C_Mh(hx, My)."""
    return (_PairwiseCostL1 if _ground(ground_cost) else _PairwiseCost).apply(
        _flat2(x), _flat2(y), _feat(hy), _feat(Mx), _feat(hx), _feat(My), float(scaling_coef))


def _solve(C, epsilon, L, Lmin, stop_mode, tag):
    return _Sinkhorn.apply(C.unsqueeze(0), float(epsilon), int(L), int(Lmin), stop_mode, tag)[0]


def benchmark_sinkhorn(x, y, scaling_coef, epsilon=1.0, L=10, Lmin=10, *, ground_cost="l2"):
    """gan_utils.py:75-121.  Sinkhorn on the plain cost_xy; the stop rule tests the loop INDEX
    against Lmin (gan_utils.py:116)."""
    return _solve(cost_xy(x, y, scaling_coef, ground_cost=ground_cost), epsilon, L, Lmin, _lib.STOP_INDEX,
                  "benchmark_sinkhorn")


def compute_sinkhorn(x, y, hy, Mx, scaling_coef, hx=None, My=None, epsilon=1.0, L=100, bi_causal=False, *,
                     ground_cost="l2"):
    """gan_utils.py:124-165.  Lmin = 100 is hard-coded in the reference (gan_utils.py:149)."""
    if bi_causal:
        C = bi_causal_modified_cost(x, y, hy, Mx, hx, My, scaling_coef, ground_cost=ground_cost)
    else:
        C = modified_cost(x, y, hy, Mx, scaling_coef, ground_cost=ground_cost)
    return _solve(C, epsilon, L, _LMIN, _lib.STOP_COUNT, "compute_sinkhorn")


def compute_N(M):
    """gan_utils.py:168-176 (unused by the reference's training loop)."""
    T = M.shape[1]
    return M[:, 1:] - M[:, :T - 1]


def scale_invariante_martingale_regularization(M, reg_lam, scaling_coef):
    """gan_utils.py:179-201."""
    return _Martingale.apply(_feat(M), float(reg_lam), float(scaling_coef))


def _loss_inputs(videos, feats, sinkhorn_eps, sinkhorn_l, honor_eps_l):
    """Prologue of the compute_*_loss functions: the videos as [B, K] (``video=True`` or not, both layouts flatten the
    same way), the features as fp32 [B, T, J], and (epsilon, L) = (1.0, 100) unless honor_eps_l (compute_sinkhorn_loss)."""
    eps, L = (float(sinkhorn_eps), int(sinkhorn_l)) if honor_eps_l else (1.0, 100)
    return [_flat2(v) for v in videos], [_feat(t) for t in feats], eps, L


def compute_sinkhorn_loss(f_real, f_fake, scaling_coef, sinkhorn_eps, sinkhorn_l, h_fake, m_real, h_real,
                          m_fake, video=True, *, honor_eps_l=False, ground_cost="l2"):
    """gan_utils.py:204-227: 2*W(real,fake) - W(real,real) - W(fake,fake).

    As in the reference, ``sinkhorn_eps`` and ``sinkhorn_l`` are accepted and IGNORED: the
    reference passes them positionally into the ``hx`` / ``My`` slots of ``compute_sinkhorn``
    (gan_utils.py:221-223 vs :124), which are unused when bi_causal=False, so the loss always
    runs with epsilon = 1.0 and L = 100.  ``honor_eps_l=True`` (keyword-only, not in the
    reference) opts into the documented intent instead.

    ``video=True`` inputs are [B,H,T,W,C]; the reference's transpose(0,2,1,3,4)+reshape
    (gan_utils.py:217-220) does not change a sum over all of (T,H,W,C), so the buffer is read as is.

    ``ground_cost="l1"`` (keyword-only, not in the reference): the three cost matrices carry the L1 distance instead of
    the squared one; the solves, the combination and what ``last_info`` records are the same.
    """
    l1 = _ground(ground_cost)
    vids, feats, eps, L = _loss_inputs((f_real, f_fake), (h_fake, h_real, m_real, m_fake), sinkhorn_eps, sinkhorn_l,
                                       honor_eps_l)
    if l1:      # the cost stage with COST_L1 and its own adjoint, then the divergence on any cost matrices
        C3 = _Cost3L1.apply(*vids, *feats, float(scaling_coef))
        loss = _SinkhornDivergence.apply(C3, eps, L, _LMIN, "compute_sinkhorn_loss")      # counts, executed counts, costs
        last_info["compute_sinkhorn_loss_C3"], last_info["compute_sinkhorn_loss_fused_sweep"] = C3.detach(), False
        return loss
    # one library call each way; equivalent to _Cost3 (C3 = [xy, xx, yy]) followed by _SinkhornDivergence
    return _SinkhornLoss.apply(_ONE_BATCH, "compute_sinkhorn_loss", float(scaling_coef), eps, L, _LMIN, *vids, *feats,
                               None, None)


def compute_mixed_sinkhorn_loss(f_real, f_fake, f_real_p, f_fake_p, scaling_coef, sinkhorn_eps, sinkhorn_l,
                                h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p, video=True, *, honor_eps_l=False):
    """Mixed Sinkhorn divergence of COT-GAN over two minibatches of real (x, x') and generated (y, y') data:

        loss = (W(x, y) + W(x', y')) - W(x, x') - W(y, y')

    with W = compute_sinkhorn (gan_utils.py:124, bi_causal=False) and the (h, M) pairs
    W(x,y; h_fake, m_real), W(x',y'; h_fake_p, m_real_p), W(x,x'; h_real_p, m_real), W(y,y'; h_fake_p, m_fake)
    (h indexes rows, M columns).  EXTENSION: the reference describes this estimator in the docstring of
    compute_sinkhorn_loss (gan_utils.py:207-208) and names it in kernel_train.py's ``--mixed_sinkhorn`` flag, but
    evaluates only the one-batch form.  With x' = x, y' = y, h_fake_p = h_fake, m_real_p = m_real, h_real_p = h_real
    it equals compute_sinkhorn_loss(f_real, f_fake, ..., h_fake, m_real, h_real, m_fake) term by term.

    ``sinkhorn_eps`` / ``sinkhorn_l`` are ignored by default (epsilon = 1, L = 100) exactly as in compute_sinkhorn_loss;
    ``honor_eps_l=True`` applies them.  Differentiable w.r.t. the fake videos and all six features; a real video that
    requires a gradient raises NotImplementedError.  Records last_info["compute_mixed_sinkhorn_loss"] (the four
    reference-equivalent iteration counts), ``..._executed``, ``..._costs`` [4] and ``..._Cmix`` [4,B,B].
    """
    vids, feats, eps, L = _loss_inputs((f_real, f_fake, f_real_p, f_fake_p),
                                       (h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p), sinkhorn_eps, sinkhorn_l,
                                       honor_eps_l)
    if any(v.shape != vids[0].shape for v in vids[1:]):
        raise ValueError("the four videos must have the same shape: %s" % ([tuple(v.shape) for v in vids],))
    if any(t.shape != feats[0].shape for t in feats[1:]) or feats[0].shape[0] != vids[0].shape[0]:
        raise ValueError("the six features must all be [B,T,J] with the videos' B; got %s" % ([tuple(t.shape) for t in feats],))
    # stacked minibatches (2 B K floats copied); cat's backward hands d[y; y'] back to y and y' as two views
    R = torch.cat([vids[0], vids[2]], 0)
    F = torch.cat([vids[1], vids[3]], 0)
    return _SinkhornLoss.apply(_MIXED, "compute_mixed_sinkhorn_loss", float(scaling_coef), eps, L, _LMIN, R, F, *feats,
                               None, None)


def compute_bicausal_sinkhorn_loss(f_real, f_fake, scaling_coef, sinkhorn_eps, sinkhorn_l, h_fake, m_real, h_real,
                                   m_fake, video=True, *, honor_eps_l=False, ground_cost="l2"):
    """Bi-causal Sinkhorn loss, 2 W(x,y) - W(x,x) - W(y,y) with W = compute_sinkhorn(..., bi_causal=True)
    (gan_utils.py:124-136) and x = real, y = fake:

        W(x,y) = compute_sinkhorn(real, fake, h_fake, m_real, sc, hx=h_real, My=m_fake, bi_causal=True)
        W(x,x) = compute_sinkhorn(real, real, h_real, m_real, sc, hx=h_real, My=m_real, bi_causal=True)
        W(y,y) = compute_sinkhorn(fake, fake, h_fake, m_fake, sc, hx=h_fake, My=m_fake, bi_causal=True)

    i.e. C_xy gains the causal term of (h_real rows, m_fake columns) and C_xx / C_yy carry their own causal term twice.
    EXTENSION: the reference implements the bi-causal cost and names the mode in kernel_train.py's ``--bi_causal`` flag
    (:396), but its compute_sinkhorn_loss never passes ``bi_causal``.  Same positional arguments as compute_sinkhorn_loss;
    ``sinkhorn_eps`` / ``sinkhorn_l`` are ignored by default (epsilon = 1, L = 100) for the same reason, and
    ``honor_eps_l=True`` applies them.  Differentiable w.r.t. the fake videos and all four features; a real video that
    requires a gradient raises NotImplementedError.  Records last_info["compute_bicausal_sinkhorn_loss"] (the three
    reference-equivalent iteration counts), ``..._executed``, ``..._costs`` [3], ``..._C3`` [3,B,B] and
    ``..._fused_sweep``.  ``ground_cost`` is here because the parameter list is compute_sinkhorn_loss's: only "l2" runs, the
    bi-causal loss has no L1 form ("l1" raises NotImplementedError).
    """
    if _ground(ground_cost):
        raise NotImplementedError("compute_bicausal_sinkhorn_loss has no L1 form; ground_cost='l1' is compute_sinkhorn_loss's")
    vids, feats, eps, L = _loss_inputs((f_real, f_fake), (h_fake, h_real, m_real, m_fake), sinkhorn_eps, sinkhorn_l,
                                       honor_eps_l)
    return _SinkhornLoss.apply(_BICAUSAL, "compute_bicausal_sinkhorn_loss", float(scaling_coef), eps, L, _LMIN, *vids, *feats,
                               None, None)


def compute_weighted_sinkhorn(x, y, hy, Mx, scaling_coef, mu, nu, epsilon=1.0, L=100):
    """compute_sinkhorn (gan_utils.py:124-165, bi_causal=False) with marginals ``mu`` over the rows (the samples of x) and
    ``nu`` over the columns (the samples of y) instead of 1/n: the updates subtract from log mu_i / log nu_j.
    EXTENSION: the reference hard-codes the uniform marginals (gan_utils.py:138-139).  ``mu`` / ``nu``: [n] device tensors,
    strictly positive, finite and normalised by the caller.  Differentiable w.r.t. x, y, hy, Mx AND mu, nu (the reverse sweep
    sums the adjoints of the duals it holds anyway: include/kccot_weight_grad.h; the gradient is that of the cost as a
    function of unconstrained weights, not projected onto sum = 1).  With mu = nu = 1/n this is compute_sinkhorn to rounding.  A weight that is <= 0 or not
    finite gives a NaN cost and a negative count in last_info["compute_weighted_sinkhorn"] (raise_if_solver_aborted
    reports it).  n <= 128 runs the register-resident kernels, larger n the streaming single-workgroup solver; the multi-CU
    solver is not weighted and never used here (last_info["compute_weighted_sinkhorn_path"])."""
    C = modified_cost(x, y, hy, Mx, scaling_coef)
    n = C.shape[0]
    if C.shape[1] != n:
        raise ValueError("the weighted solver needs as many samples in x as in y; got %s" % (tuple(C.shape),))
    a, b = _weights(mu, n, "mu", False), _weights(nu, n, "nu", False)
    return _WeightedSinkhorn.apply(C.unsqueeze(0), a.unsqueeze(0), b.unsqueeze(0), float(epsilon), int(L), _LMIN,
                                   _lib.STOP_COUNT, "compute_weighted_sinkhorn")[0]


def compute_weighted_sinkhorn_loss(f_real, f_fake, scaling_coef, sinkhorn_eps, sinkhorn_l, h_fake, m_real, h_real,
                                   m_fake, w_real, w_fake, video=True, normalize=True):
    """The one-batch causal loss with weighted samples,

        2 W(C_xy; a, b) - W(C_xx; a, a) - W(C_yy; b, b),   a = w_real, b = w_fake,

    with the three cost matrices of compute_sinkhorn_loss and W the Sinkhorn cost whose marginals are a over the rows and
    b over the columns (compute_weighted_sinkhorn).  EXTENSION, not reference behaviour: the reference's solver
    hard-codes mu = nu = 1/n; this is what the kernel estimator of the conditional law, importance weights or shards of
    unequal mass need.  With uniform weights it is compute_sinkhorn_loss(..., honor_eps_l=True) to rounding.

    ``sinkhorn_eps`` and ``sinkhorn_l`` ARE applied (this function has no reference quirk to mirror).  ``w_real`` /
    ``w_fake``: [B] device tensors of strictly positive finite weights; ``normalize=True`` divides each by its sum on the
    device (no host synchronisation), ``normalize=False`` takes them as given.  Differentiable w.r.t. the fake videos, the
    four features and the two weight vectors (through the normalisation, which is a torch division; the weight gradients
    come from kccot_weighted_sinkhorn_loss_bwd_dw_f32 and are computed only when asked for: the other gradients are the same
    bits either way); a real video that requires a gradient raises NotImplementedError.  Always the
    dual-history path: the one-launch fused loss and the multi-CU solver are not weighted.  Records
    last_info["compute_weighted_sinkhorn_loss"] (three counts; negative = a bad weight poisoned that problem, its cost
    and the gradients are NaN), ``..._executed``, ``..._costs`` [3], ``..._C3`` [3,B,B], ``..._fused_sweep`` (False) and
    ``..._path`` ("register" for B <= 128, "streaming" above)."""
    vids, feats, eps, L = _loss_inputs((f_real, f_fake), (h_fake, h_real, m_real, m_fake), sinkhorn_eps, sinkhorn_l, True)
    B = vids[0].shape[0]
    a, b = _weights(w_real, B, "w_real", normalize), _weights(w_fake, B, "w_fake", normalize)
    return _SinkhornLoss.apply(_WEIGHTED, "compute_weighted_sinkhorn_loss", float(scaling_coef), eps, L, _LMIN, *vids, *feats,
                               a, b)


def _query_rows(c, queries, who):
    """The rows of the context c [B, Kc] that ``queries`` names (None: all B, in order), within the weight estimator's limit
    on B."""
    if c.shape[0] > 1024:
        raise NotImplementedError("%s: B=%d > 1024" % (who, c.shape[0]))
    if queries is None:
        return c
    queries = torch.as_tensor(queries, device=c.device)
    if queries.dim() != 1 or queries.numel() < 1 or queries.dtype not in (torch.int32, torch.int64):
        raise ValueError("queries must be a non-empty 1-D integer index tensor")
    return c.index_select(0, queries.long()).contiguous()


def _check_query_weights(query_weights, Q):
    """``query_weights`` is None or [Q] (_gpu_f32 then makes it what the library reads)."""
    if query_weights is not None and tuple(query_weights.shape) != (Q,):
        raise ValueError("query_weights must be [%d], got %s" % (Q, tuple(query_weights.shape)))


def kernel_conditional_weights(context, bandwidth, queries=None):
    """Gaussian-kernel estimate of the conditional law, one row per query: EXTENSION, not reference behaviour (the
    weights compute_conditional_sinkhorn_loss takes).  ``context``: [B, ...] on the device, read as [B, Kc]; ``queries``:
    an index tensor of Q samples of the batch (default: all B, in order).  With D[q,i] = |c_q - c_i|^2 (cost_xy with
    scaling_coef = 1) row q is

        w[q,i] = max(softmax_i(-D[q,i] / (2 bandwidth^2)), 2^-100)      (kccot_conditional_weights_f32)

    -- the floor keeps a peaked kernel from handing the solver a zero weight; rows are not renormalised after it.  Returns
    [Q, B] fp32.  The weights are not differentiated here: a context that requires a gradient raises NotImplementedError --
    compute_kernel_conditional_sinkhorn_loss is the differentiable form (context, bandwidth and query weights)."""
    if not torch.is_tensor(context) or context.dim() < 2:
        raise ValueError("context must be a tensor [batch, ...]")
    if context.requires_grad:
        raise NotImplementedError("kernel_conditional_weights does not differentiate w.r.t. the context; detach it, or use "
                                  "compute_kernel_conditional_sinkhorn_loss, which does")
    if not float(bandwidth) > 0.0:
        raise ValueError("bandwidth must be > 0 (got %r)" % (bandwidth,))
    c = _flat2(context)
    with torch.no_grad():
        D = cost_xy(_query_rows(c, queries, "kernel_conditional_weights"), c, 1.0).contiguous()
    Q, B = D.shape
    w = _lib.empty((Q, B), torch.float32, c.device)
    check(lib.kccot_conditional_weights_f32(ptr(D), Q, B, float(bandwidth), ptr(w), stream_of(D)), "conditional_weights")
    return w


def compute_conditional_sinkhorn_loss(f_real, f_fake, scaling_coef, sinkhorn_eps, sinkhorn_l, h_fake, m_real, h_real,
                                      m_fake, weights, query_weights=None, video=True):
    """The kernel-conditional causal loss: Q weighted solves of the one-batch loss on ONE shared set of cost matrices,

        loss = sum_q omega_q (2 W(C_xy; w_q, w_q) - W(C_xx; w_q, w_q) - W(C_yy; w_q, w_q)),

    with the three cost matrices of compute_sinkhorn_loss, W the weighted Sinkhorn cost (compute_weighted_sinkhorn),
    w_q = ``weights[q]`` the estimate of the conditional law given the context of query q (kernel_conditional_weights; real
    sample i and fake sample i share context i, so both marginals of all three problems are w_q) and omega =
    ``query_weights`` ([Q]; None: 1/Q).  EXTENSION, not reference behaviour: the reference evaluates the loss with uniform
    marginals only.  One library call each way (include/kccot_conditional.h): the cost matrices are assembled once, the
    3 Q solves run as one launch (one workgroup each), loss and gradient are accumulated in double in ascending q.

    ``sinkhorn_eps`` and ``sinkhorn_l`` ARE applied, as in compute_weighted_sinkhorn_loss.  ``weights``: [Q, B] device
    tensor, strictly positive and finite, rows normalised by the caller.  Differentiable w.r.t. the fake videos and the
    four features; a real video or a weight tensor that requires a gradient raises NotImplementedError
    (compute_kernel_conditional_sinkhorn_loss differentiates w.r.t. the context, the bandwidth and the query weights).  Records
    last_info["compute_conditional_sinkhorn_loss"] (counts [Q,3]; a negative row = a bad weight poisoned that query: its
    costs, the loss and the gradients are NaN), ``..._executed`` [Q,3], ``..._costs`` [Q,3], ``..._C3`` [3,B,B],
    ``..._path`` ("register" for B <= 128, "streaming" above) and ``..._fused_sweep`` (False)."""
    for name, t in (("weights", weights), ("query_weights", query_weights)):
        if t is not None and not torch.is_tensor(t):
            raise TypeError("%s must be a tensor" % name)
        if t is not None and t.requires_grad:
            raise NotImplementedError("%s: the conditional Sinkhorn loss does not differentiate w.r.t. the weights; "
                                      "compute_kernel_conditional_sinkhorn_loss does" % name)
    if torch.is_tensor(f_real) and f_real.requires_grad:
        raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
    if weights.dim() != 2 or weights.shape[0] < 1:
        raise ValueError("weights must be [Q, B] with Q >= 1, got %s" % (tuple(weights.shape),))
    _check_query_weights(query_weights, weights.shape[0])
    vids, feats, eps, L = _loss_inputs((f_real, f_fake), (h_fake, h_real, m_real, m_fake), sinkhorn_eps, sinkhorn_l, True)
    B = vids[0].shape[0]
    if weights.shape[1] != B:
        raise ValueError("weights must be [Q, %d], got %s" % (B, tuple(weights.shape)))
    return _SinkhornLoss.apply(_CONDITIONAL, "compute_conditional_sinkhorn_loss", float(scaling_coef), eps, L, _LMIN, *vids,
                               *feats, _gpu_f32(weights), _gpu_f32(query_weights))


def compute_kernel_conditional_sinkhorn_loss(f_real, f_fake, scaling_coef, sinkhorn_eps, sinkhorn_l, h_fake, m_real, h_real,
                                             m_fake, context, bandwidth, queries=None, query_weights=None, video=True):
    """kernel_conditional_weights and compute_conditional_sinkhorn_loss in ONE differentiable call:

        loss = sum_q omega_q (2 W(C_xy; w_q, w_q) - W(C_xx; w_q, w_q) - W(C_yy; w_q, w_q)),
        w_q  = max(softmax_i(-|c_q - c_i|^2 / (2 bandwidth^2)), 2^-100),      c = ``context`` [B, ...], q over ``queries``

    EXTENSION, not reference behaviour.  Differentiable w.r.t. the fake videos and the four features (as
    compute_conditional_sinkhorn_loss), and w.r.t. what that pair of functions refuses:
      * ``query_weights`` [Q]:  dloss/domega_q is the loss of query q;
      * ``bandwidth`` when it is a 0-dim fp32 device tensor (it is then read on the device, never on the host, so a step can
        be captured; it must be > 0, else the weights are NaN and the solver reports them).  A Python float is a constant;
      * ``context``: dloss/dw [Q,B] (the reverse sweeps' sums of dual adjoints, include/kccot_weight_grad.h) -> the adjoint
        of the kernel estimator (floored entries have zero slope) -> the squared distances' backward, on the query side and
        on the sample side.
    The weight gradient is computed only when one of the three asks for it.  With nothing new requiring a gradient the result
    and the other gradients are, bit for bit, those of compute_conditional_sinkhorn_loss(..., kernel_conditional_weights(
    context, bandwidth, queries), query_weights).  A real video that requires a gradient raises NotImplementedError.  Records
    the keys of compute_conditional_sinkhorn_loss under last_info["compute_kernel_conditional_sinkhorn_loss"...]."""
    tag = "compute_kernel_conditional_sinkhorn_loss"
    if not torch.is_tensor(context) or context.dim() < 2:
        raise ValueError("context must be a tensor [batch, ...]")
    if query_weights is not None and not torch.is_tensor(query_weights):
        raise TypeError("query_weights must be a tensor")
    if torch.is_tensor(f_real) and f_real.requires_grad:
        raise NotImplementedError("the loss path never differentiates w.r.t. real (kernel_train.py:252,289)")
    if torch.is_tensor(bandwidth):
        if bandwidth.dim() != 0:
            raise ValueError("a tensor bandwidth must be 0-dim, got shape %s" % (tuple(bandwidth.shape),))
    elif not float(bandwidth) > 0.0:
        raise ValueError("bandwidth must be > 0 (got %r)" % (bandwidth,))
    vids, feats, eps, L = _loss_inputs((f_real, f_fake), (h_fake, h_real, m_real, m_fake), sinkhorn_eps, sinkhorn_l, True)
    B = vids[0].shape[0]
    c = _flat2(context)
    if c.shape[0] != B:
        raise ValueError("context must have the videos' batch size %d, got %d" % (B, c.shape[0]))
    cq = _query_rows(c, queries, tag)
    _check_query_weights(query_weights, cq.shape[0])
    omega = _gpu_f32(query_weights)
    bw = _gpu_f32(bandwidth) if torch.is_tensor(bandwidth) else float(bandwidth)
    w = _KernelWeights.apply(cost_xy(cq, c, 1.0).contiguous(), bw)
    return _SinkhornLoss.apply(_CONDITIONAL, tag, float(scaling_coef), eps, L, _LMIN, *vids, *feats, w, omega)


def raise_if_solver_aborted(tags=("compute_sinkhorn_loss",)):
    """Synchronising status check of the solves recorded under ``tags`` in ``last_info`` (``kccot_sinkhorn_status``): raises
    ``KccotError`` if a multi-CU Sinkhorn solve gave up (negative iteration count; its cost and gradients are NaN).  The
    training loop calls it where the reference has its non-finite-loss guard (kernel_train.py:323), so that an aborted
    solve is reported as what it is and not as an exploded loss.  Default: the loss the trainer just evaluated (the
    single-GPU and the batch-sharded path both record their counts under "compute_sinkhorn_loss"); pass
    ``("compute_sinkhorn",)`` / ``("benchmark_sinkhorn",)`` after a direct call of those.  Under the tags of the weighted
    solver ("compute_weighted_sinkhorn", "compute_weighted_sinkhorn_loss") and of the conditional loss
    ("compute_conditional_sinkhorn_loss", "compute_kernel_conditional_sinkhorn_loss", counts [Q,3]) a negative count means a weight that was <= 0 or not finite, and
    the error says so.  A checked entry is dropped, so a stale record of an earlier call can never be
    blamed for a later NaN."""
    for tag in tags:
        nits = last_info.pop(tag, None)
        if nits is None or not torch.is_tensor(nits) or not nits.is_cuda:
            continue
        nits = nits.contiguous().reshape(-1)
        rc = 0
        for lo in range(0, int(nits.numel()), 4096):      # kccot_sinkhorn_status reads at most 4096 counts per call
            part = nits[lo:lo + 4096]
            rc = rc or lib.kccot_sinkhorn_status(ptr(part), int(part.numel()), stream_of(nits))
        if rc == _lib.EABORTED:
            if tag.startswith(("compute_weighted_", "compute_conditional_", "compute_kernel_conditional_")):     # never multi-CU: the only cause
                raise _lib.KccotError("%s: a marginal weight of a problem was <= 0 or not finite; its cost and gradients "
                                      "are NaN (counts %s)" % (tag, nits.tolist()))
            raise _lib.KccotError("%s: %s" % (tag, lib.kccot_last_error().decode("utf-8", "replace")))
        check(rc, "sinkhorn_status")
