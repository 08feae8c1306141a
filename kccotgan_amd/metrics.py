"""EXTENSION -- not reference behaviour.  The reference publishes no sample-quality figure ("none
published"); these are the two per-frame numbers every video-prediction paper reports, SSIM and PSNR, of a generated video
against the ground truth, both [B,H,T,W,C].  The definition (Wang et al. 2004 with a Gaussian window and VALID borders: what
scikit-image computes with ``gaussian_weights=True, use_sample_covariance=False``, on this library's fp32 taps) and the adjoint
are in ``include/kccot_metrics.h``; the kernels are in ``csrc/ssim.hip``: one fused walk each way, no tensor-sized intermediate.

``ssim`` is differentiable w.r.t. ``fake`` (1 - SSIM is a common auxiliary loss term) and, as everywhere on the loss path, never
w.r.t. ``real``.  GPU tensors only: there is no CPU path.
"""
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_of, workspace, require_gpu

DEFAULT_WIN, DEFAULT_SIGMA = 11, 1.5


def _window(real, fake, data_range, win_size, sigma):
    """The Python-side argument rules; returns the radius."""
    if real.dim() != 5 or real.shape != fake.shape:
        raise ValueError("metrics: real and fake must be [B,H,T,W,C] of one shape (got %s and %s)"
                         % (tuple(real.shape), tuple(fake.shape)))
    if int(win_size) != win_size or win_size % 2 == 0 or not 1 <= win_size <= 15:
        raise ValueError("metrics: win_size must be odd and in 1..15 (got %r)" % (win_size,))
    if win_size > real.shape[1] or win_size > real.shape[3]:
        raise ValueError("metrics: a window of %d does not fit a %d x %d frame" % (win_size, real.shape[1], real.shape[3]))
    if not float(sigma) > 0 or not float(data_range) > 0:
        raise ValueError("metrics: sigma and data_range must be > 0 (got %r, %r)" % (sigma, data_range))
    return int(win_size) // 2


def _dense(v):
    require_gpu(v)
    return v.detach().float().contiguous()


def _forward(real, fake, data_range, radius, sigma, want_mse):
    B, H, T, W, C = real.shape
    s = _lib.empty((B, T), torch.float32, real.device)
    m = _lib.empty((B, T), torch.float32, real.device) if want_mse else None
    ws, wsb = workspace(lib.kccot_ssim_workspace_bytes(B, H, T, W, C), real)
    check(lib.kccot_ssim_fwd_f32(ptr(real), ptr(fake), B, H, T, W, C, float(sigma), radius, float(data_range), ptr(s), ptr(m),
                                 ws, wsb, stream_of(real)), "ssim_fwd")
    return s, m


class _SSIM(torch.autograd.Function):
    """Nothing but real and fake is kept for the backward: it recomputes the moments."""

    @staticmethod
    def forward(ctx, real, fake, data_range, radius, sigma):
        x, y = _dense(real), _dense(fake)
        ctx.save_for_backward(x, y)
        ctx.cfg = (float(data_range), radius, float(sigma), fake.dtype)
        return _forward(x, y, data_range, radius, sigma, False)[0]

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("ssim differentiates w.r.t. fake only (the loss path never needs d/d real)")
        x, y = ctx.saved_tensors
        data_range, radius, sigma, dtype = ctx.cfg
        B, H, T, W, C = x.shape
        g = g.float().contiguous()
        dy = _lib.empty_like(y)
        ws, wsb = workspace(lib.kccot_ssim_workspace_bytes(B, H, T, W, C), x)
        check(lib.kccot_ssim_bwd_f32(ptr(g), ptr(x), ptr(y), B, H, T, W, C, sigma, radius, data_range, ptr(dy), ws, wsb,
                                     stream_of(x)), "ssim_bwd")
        return None, dy.to(dtype), None, None, None


def ssim(real, fake, data_range=1.0, win_size=DEFAULT_WIN, sigma=DEFAULT_SIGMA):
    """[B,T]: the mean structural similarity of every frame of ``fake`` against ``real`` over the (H - win_size + 1) x
    (W - win_size + 1) window positions and the channels.  Differentiable w.r.t. ``fake``; a gradient w.r.t. ``real`` raises
    NotImplementedError.  ``win_size`` is odd, 1..15, and no larger than the frame (ValueError)."""
    radius = _window(real, fake, data_range, win_size, sigma)
    return _SSIM.apply(real, fake, data_range, radius, sigma)


def _psnr_of(mse, data_range):
    return 10.0 * torch.log10(float(data_range) ** 2 / mse)         # mse == 0: +inf


def frame_metrics(real, fake, data_range=1.0, win_size=DEFAULT_WIN, sigma=DEFAULT_SIGMA):
    """(ssim [B,T], psnr [B,T]) from ONE forward call; no tape."""
    radius = _window(real, fake, data_range, win_size, sigma)
    with torch.no_grad():
        s, m = _forward(_dense(real), _dense(fake), data_range, radius, sigma, True)
        return s, _psnr_of(m, data_range)


def psnr(real, fake, data_range=1.0):
    """[B,T]: 10 log10(data_range^2 / mse) of every frame, mse the mean of (real - fake)^2 over H, W and C (the differences in
    fp32, the sum in fp64); identical frames give +inf.  No tape.  The mean squared error comes out of the SSIM walk, so this is
    ``frame_metrics`` at its default window (at win_size 1 where the frame is smaller than that) with the SSIM dropped: the same
    bits as ``frame_metrics(real, fake, data_range)[1]``."""
    fits = real.dim() == 5 and min(real.shape[1], real.shape[3]) >= DEFAULT_WIN
    return frame_metrics(real, fake, data_range, DEFAULT_WIN if fits else 1, DEFAULT_SIGMA)[1]
