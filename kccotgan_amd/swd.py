"""EXTENSION -- not reference behaviour.  The squared sliced Wasserstein distance (order 2) between two batches: an optimal-
transport distance between the real and the generated *distribution* with no epsilon, no bandwidth and no learned features, so
its value can be compared across runs.  The definition, the generator of the directions and the arithmetic are in
``include/kccot_swd.h``; the kernels are in ``csrc/swd.hip``.  The directions are never stored: the kernels generate them on chip
from ``seed``, forward and backward.

``sliced_wasserstein2`` is differentiable w.r.t. both batches; the gradient w.r.t. ``real`` is computed only when autograd asks
for it.  GPU tensors only: there is no CPU path.
"""
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_of, workspace, require_gpu

MAX_B, MAX_P = 1024, 65535


def _rows(real, fake, n_projections, seed):
    """The Python-side argument rules; returns (B, K, P, seed)."""
    if real.dim() < 2 or real.shape != fake.shape:
        raise ValueError("swd: real and fake must be [B,...] of one shape (got %s and %s)" % (tuple(real.shape), tuple(fake.shape)))
    if int(n_projections) != n_projections or not 1 <= n_projections <= MAX_P:
        raise ValueError("swd: n_projections must be an integer in 1..%d (got %r)" % (MAX_P, n_projections))
    if int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("swd: seed must be an integer in 0..2^64-1 (got %r)" % (seed,))
    B = int(real.shape[0])
    if B < 1 or real.numel() < 1:
        raise ValueError("swd: empty batch %s" % (tuple(real.shape),))
    K = real.numel() // B
    if B > MAX_B:
        raise NotImplementedError("swd: B=%d > %d" % (B, MAX_B))
    return B, K, int(n_projections), int(seed)


def _dense(v, B, K):
    require_gpu(v)
    return v.detach().float().contiguous().view(B, K)


class _SWD(torch.autograd.Function):
    """Saves proj / order / inv_norm ([2,P,B] and [P]); neither video is kept for the backward."""

    @staticmethod
    def forward(ctx, real, fake, P, seed):
        B = int(real.shape[0])
        K = real.numel() // B
        x, y = _dense(real, B, K), _dense(fake, B, K)
        proj = _lib.empty((2, P, B), torch.float32, x.device)
        order = _lib.empty((2, P, B), torch.int32, x.device)
        inv_norm = _lib.empty((P,), torch.float32, x.device)
        out = _lib.empty((1,), torch.float32, x.device)
        ws, wsb = workspace(lib.kccot_swd_workspace_bytes(B, K, P), x)
        check(lib.kccot_swd_fwd_f32(ptr(x), ptr(y), B, K, P, seed, ptr(proj), ptr(order), ptr(inv_norm), ptr(out), ws, wsb,
                                    stream_of(x)), "swd_fwd")
        ctx.save_for_backward(proj, order, inv_norm)
        ctx.cfg = (B, K, P, seed, tuple(real.shape), real.dtype, fake.dtype)
        return out.view(())

    @staticmethod
    def backward(ctx, g):
        proj, order, inv_norm = ctx.saved_tensors
        B, K, P, seed, shape, rdtype, fdtype = ctx.cfg
        g = g.detach().float().contiguous().view(1)
        dreal = _lib.empty((B, K), torch.float32, proj.device) if ctx.needs_input_grad[0] else None
        dfake = _lib.empty((B, K), torch.float32, proj.device) if ctx.needs_input_grad[1] else None
        if dreal is None and dfake is None:
            return None, None, None, None
        ws, wsb = workspace(lib.kccot_swd_workspace_bytes(B, K, P), proj)
        check(lib.kccot_swd_bwd_f32(ptr(g), ptr(proj), ptr(order), ptr(inv_norm), B, K, P, seed, ptr(dreal), ptr(dfake), ws, wsb,
                                    stream_of(proj)), "swd_bwd")
        return (None if dreal is None else dreal.view(shape).to(rdtype), None if dfake is None else dfake.view(shape).to(fdtype),
                None, None)


def sliced_wasserstein2(real, fake, n_projections=128, seed=0):
    """A scalar: SW2 = 1 / (P B) sum_p sum_r (a_(r),p - b_(r),p)^2 of ``real`` against ``fake`` (both [B,...], flattened to
    [B,K]; B <= 1024) on ``n_projections`` (<= 65535) random directions drawn from ``seed`` (an integer below 2^64; the same
    seed gives the same directions, and direction p depends on neither P nor K).  The square, not its root.  Differentiable
    w.r.t. ``fake`` and ``real``."""
    B, K, P, seed = _rows(real, fake, n_projections, seed)
    return _SWD.apply(real, fake, P, seed)


def directions(seed, K, p_begin, p_count, device="cuda"):
    """[p_count, K] float32: the raw (un-normalised) directions p_begin .. p_begin + p_count - 1 of ``seed``, as the kernels
    generate them (for tests and for reproducing a value elsewhere)."""
    if int(seed) != seed or not 0 <= seed < 1 << 64:
        raise ValueError("swd: seed must be an integer in 0..2^64-1 (got %r)" % (seed,))
    if K < 1 or p_count < 1 or p_begin < 0 or p_begin + p_count > MAX_P:
        raise ValueError("swd: directions need K >= 1 and 0 <= p_begin, p_count >= 1, p_begin + p_count <= %d (got %r, %r, %r)"
                         % (MAX_P, K, p_begin, p_count))
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.KccotError("kccotgan_amd needs a ROCm device (got %s); there is no CPU path" % device)
    out = _lib.empty((int(p_count), int(K)), torch.float32, device)
    check(lib.kccot_swd_directions_f32(int(seed), int(K), int(p_begin), int(p_count), ptr(out), stream_of(out)), "swd_directions")
    return out
