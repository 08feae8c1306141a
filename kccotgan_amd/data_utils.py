"""Drop-in for the ``KernelSmoothing`` class of the reference's ``data_utils.py`` (:478-586):
Gaussian smoothing of [B,H,T,W,C] videos by the HIP kernels behind ``include/kccot.h``.

Only the part of ``data_utils.py`` that sits on the loss path is mirrored; dataset loaders,
plotting and learning-rate schedules are out of scope.
"""
import torch

from . import _lib
from ._lib import lib, check, ptr, stream_of, workspace

__all__ = ["KernelSmoothing"]


CAUSAL3 = "causal3"     # `axes` of the causal 3-D smoothing: its own entry points (include/kccot_smooth_causal3.h), protocol flags only


def _entry(axes):
    """(forward, backward, sharded backward, axis flags) for an `axes` value."""
    if axes == CAUSAL3:
        return lib.kccot_smooth_causal3_fwd_f32, lib.kccot_smooth_causal3_bwd_f32, lib.kccot_smooth_causal3_bwd_sharded_f32, 0
    return lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, lib.kccot_smooth_bwd_sharded_f32, axes


def _sigma_bits(axes):
    """`axes_flags` of kccot_smooth_dsigma_f32 (include/kccot_smooth_sigma.h) for an `axes` value: there the causal 3-D form
    is spelled with the axis bits."""
    if axes == CAUSAL3:
        return _lib.SMOOTH_T | _lib.SMOOTH_H | _lib.SMOOTH_W | _lib.SMOOTH_CAUSAL_T
    return axes


def _fwd(x, sigma, radius, axes):
    B, H, T, W, C = x.shape
    out = _lib.empty_like(x)
    mx = _lib.empty((1,), torch.float32, x.device)
    ws, wsb = workspace(lib.kccot_smooth_workspace_bytes(B, H, T, W, C), x)
    fwd, _, _, bits = _entry(axes)
    check(fwd(ptr(x), B, H, T, W, C, sigma, radius, bits, ptr(out), ptr(mx), ws, wsb, stream_of(x)), "smooth_fwd")
    return out, mx


def _bwd(g, out, mx, sigma, radius, axes):
    B, H, T, W, C = out.shape
    din = _lib.empty_like(out)
    ws, wsb = workspace(lib.kccot_smooth_workspace_bytes(B, H, T, W, C), out)
    _, bwd, _, bits = _entry(axes)
    check(bwd(ptr(g), ptr(out), ptr(mx), B, H, T, W, C, sigma, radius, bits, ptr(din), ws, wsb, stream_of(out)),
          "smooth_bwd")
    return din


def _fwd_sharded(x, sigma, radius, axes, group):
    import torch.distributed as dist
    B, H, T, W, C = x.shape
    out = _lib.empty_like(x)
    mx = _lib.empty((1,), torch.float32, x.device)
    ws, wsb = workspace(lib.kccot_smooth_workspace_bytes(B, H, T, W, C), x)
    fwd, _, _, bits = _entry(axes)
    check(fwd(ptr(x), B, H, T, W, C, sigma, radius, bits | _lib.SMOOTH_NO_DIVIDE, ptr(out), ptr(mx), ws, wsb, stream_of(x)),
          "smooth_fwd")
    _all_reduce(mx, dist.ReduceOp.MAX, group)
    check(fwd(ptr(x), B, H, T, W, C, sigma, radius, bits | _lib.SMOOTH_EXTERNAL_MAX, ptr(out), ptr(mx), ws, wsb,
              stream_of(x)), "smooth_fwd")
    return out, mx


def _bwd_sharded(g, out, mx, sigma, radius, axes, group):
    """(din, the two sums of the normalisation's adjoint over the whole batch)"""
    import torch.distributed as dist
    B, H, T, W, C = out.shape
    din = _lib.empty_like(out)
    stats = _lib.empty((2,), torch.float32, out.device)
    ws, wsb = workspace(lib.kccot_smooth_workspace_bytes(B, H, T, W, C), out)
    _, _, bwd, bits = _entry(axes)
    check(bwd(ptr(g), ptr(out), ptr(mx), ptr(stats), B, H, T, W, C, sigma, radius, bits | _lib.SMOOTH_STATS_ONLY, None, ws,
              wsb, stream_of(out)), "smooth_bwd")
    _all_reduce(stats, dist.ReduceOp.SUM, group)
    check(bwd(ptr(g), ptr(out), ptr(mx), ptr(stats), B, H, T, W, C, sigma, radius, bits | _lib.SMOOTH_EXTERNAL_STATS,
              ptr(din), ws, wsb, stream_of(out)), "smooth_bwd")
    return din, stats


def _dsigma(x, g, out, mx, stats, sigma, radius, axes, like):
    """d loss / d sigma by kccot_smooth_dsigma_f32, in the shape, dtype and device of the sigma tensor `like`."""
    B, H, T, W, C = out.shape
    res = _lib.empty((1,), torch.float32, out.device)
    ws, wsb = workspace(lib.kccot_smooth_dsigma_workspace_bytes(B, H, T, W, C), out)
    check(lib.kccot_smooth_dsigma_f32(ptr(x), ptr(g), ptr(out), ptr(mx), ptr(stats), B, H, T, W, C, sigma, radius,
                                      _sigma_bits(axes), ptr(res), ws, wsb, stream_of(out)), "smooth_dsigma")
    return res.reshape(like.shape).to(device=like.device, dtype=like.dtype)


class _Smooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sigma, radius, axes):
        out, mx = _fwd(x, sigma, radius, axes)
        ctx.save_for_backward(out, mx)
        ctx.cfg = (sigma, radius, axes)
        return out

    @staticmethod
    def backward(ctx, g):
        out, mx = ctx.saved_tensors
        sigma, radius, axes = ctx.cfg
        return _bwd(g.contiguous(), out, mx, sigma, radius, axes), None, None, None


class _SmoothSharded(torch.autograd.Function):
    """The same smoothing for a batch that is sharded over the ranks of ``group`` (each rank holds B/G samples): the
    reference divides by the maximum of the WHOLE smoothed batch (data_utils.py:520,573,581), so the local maxima are
    all-reduced(MAX) before the division, and the adjoint of that division needs two sums over the whole batch
    (sum(g * out) and the number of arg-max ties), all-reduced(SUM) -- SURVEY.md section 8(e), message (4).  Results
    equal the unsharded call on the concatenated batch (tests/test_dist_gloo.py)."""

    @staticmethod
    def forward(ctx, x, sigma, radius, axes, group):
        out, mx = _fwd_sharded(x, sigma, radius, axes, group)
        ctx.save_for_backward(out, mx)
        ctx.cfg = (sigma, radius, axes, group)
        return out

    @staticmethod
    def backward(ctx, g):
        out, mx = ctx.saved_tensors
        sigma, radius, axes, group = ctx.cfg
        return _bwd_sharded(g.contiguous(), out, mx, sigma, radius, axes, group)[0], None, None, None, None


class _SmoothSigma(torch.autograd.Function):
    """_Smooth with a LEARNABLE bandwidth: ``sigma`` is a one-element tensor that requires a gradient (any device, any float
    dtype).  NOT reference behaviour (the reference anneals sigma by hand).  The forward reads the value of sigma on the
    host (``float(sigma.detach())``: a synchronisation when sigma lives on the device), so this path can NOT be captured
    into a hipGraph; out is bit-identical to the float-sigma call.  Backward: din by the same entry as _Smooth (the same
    bits), d loss / d sigma by kccot_smooth_dsigma_f32 (include/kccot_smooth_sigma.h), returned in sigma's shape, dtype and
    device.  Once differentiable."""

    @staticmethod
    def forward(ctx, x, sigma_t, radius, axes):
        sigma = float(sigma_t.detach())
        out, mx = _fwd(x, sigma, radius, axes)
        ctx.save_for_backward(x, out, mx, sigma_t)
        ctx.cfg = (sigma, radius, axes)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, out, mx, sigma_t = ctx.saved_tensors
        sigma, radius, axes = ctx.cfg
        g = g.contiguous()
        din = _bwd(g, out, mx, sigma, radius, axes) if ctx.needs_input_grad[0] else None
        ds = _dsigma(x, g, out, mx, None, sigma, radius, axes, sigma_t) if ctx.needs_input_grad[1] else None
        return din, ds, None, None


class _SmoothShardedSigma(torch.autograd.Function):
    """_SmoothSharded with a learnable bandwidth (see _SmoothSigma; sigma is replicated on every rank).  Backward: the
    stats-only pass, the all-reduce and din with the global sums as in _SmoothSharded, then kccot_smooth_dsigma_f32 with the
    GLOBAL maximum and sums over this rank's shard.  The value returned for sigma is therefore this rank's PARTIAL of
    d loss / d sigma: the sum over the ranks is the gradient of the whole batch.  That is the convention KCCOTTrainer._apply
    uses for replicated parameters (local partials, summed by the gradient all-reduce); nothing is all-reduced here."""

    @staticmethod
    def forward(ctx, x, sigma_t, radius, axes, group):
        sigma = float(sigma_t.detach())
        out, mx = _fwd_sharded(x, sigma, radius, axes, group)
        ctx.save_for_backward(x, out, mx, sigma_t)
        ctx.cfg = (sigma, radius, axes, group)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, out, mx, sigma_t = ctx.saved_tensors
        sigma, radius, axes, group = ctx.cfg
        g = g.contiguous()
        din, stats = _bwd_sharded(g, out, mx, sigma, radius, axes, group)
        ds = _dsigma(x, g, out, mx, stats, sigma, radius, axes, sigma_t) if ctx.needs_input_grad[1] else None
        return din, ds, None, None, None


# ---- the anisotropic 3-D smoothing (include/kccot_smooth_aniso.h): cfg = (sigma_t, radius_t, sigma_s, radius_s, flags)

def _aniso_ws(t):
    B, H, T, W, C = t.shape
    return workspace(lib.kccot_smooth_aniso_workspace_bytes(B, H, T, W, C), t)


def _aniso_fwd(x, cfg, group=None, sharded=False):
    st, rt, ss, rs, flags = cfg
    B, H, T, W, C = x.shape
    out = _lib.empty_like(x)
    mx = _lib.empty((1,), torch.float32, x.device)
    ws, wsb = _aniso_ws(x)

    def call(extra):
        check(lib.kccot_smooth_aniso_fwd_f32(ptr(x), B, H, T, W, C, st, rt, ss, rs, flags | extra, ptr(out), ptr(mx), ws, wsb,
                                             stream_of(x)), "smooth_aniso_fwd")
    if not sharded:
        call(0)
    else:
        import torch.distributed as dist
        call(_lib.SMOOTH_NO_DIVIDE)
        _all_reduce(mx, dist.ReduceOp.MAX, group)
        call(_lib.SMOOTH_EXTERNAL_MAX)
    return out, mx


def _aniso_bwd(g, out, mx, cfg):
    st, rt, ss, rs, flags = cfg
    B, H, T, W, C = out.shape
    din = _lib.empty_like(out)
    ws, wsb = _aniso_ws(out)
    check(lib.kccot_smooth_aniso_bwd_f32(ptr(g), ptr(out), ptr(mx), B, H, T, W, C, st, rt, ss, rs, flags, ptr(din), ws, wsb,
                                         stream_of(out)), "smooth_aniso_bwd")
    return din


def _aniso_bwd_sharded(g, out, mx, cfg, group, want_din=True):
    """(din, the two sums of the normalisation's adjoint over the whole batch)"""
    import torch.distributed as dist
    st, rt, ss, rs, flags = cfg
    B, H, T, W, C = out.shape
    stats = _lib.empty((2,), torch.float32, out.device)
    ws, wsb = _aniso_ws(out)
    bwd = lib.kccot_smooth_aniso_bwd_sharded_f32
    check(bwd(ptr(g), ptr(out), ptr(mx), ptr(stats), B, H, T, W, C, st, rt, ss, rs, flags | _lib.SMOOTH_STATS_ONLY, None, ws,
              wsb, stream_of(out)), "smooth_aniso_bwd")
    _all_reduce(stats, dist.ReduceOp.SUM, group)
    din = None
    if want_din:
        din = _lib.empty_like(out)
        check(bwd(ptr(g), ptr(out), ptr(mx), ptr(stats), B, H, T, W, C, st, rt, ss, rs, flags | _lib.SMOOTH_EXTERNAL_STATS,
                  ptr(din), ws, wsb, stream_of(out)), "smooth_aniso_bwd")
    return din, stats


def _aniso_dsigma(x, g, out, mx, stats, cfg):
    """{d loss / d sigma_t, d loss / d sigma_s} by kccot_smooth_aniso_dsigma_f32: two device floats"""
    st, rt, ss, rs, flags = cfg
    B, H, T, W, C = out.shape
    res = _lib.empty((2,), torch.float32, out.device)
    ws, wsb = _aniso_ws(out)
    check(lib.kccot_smooth_aniso_dsigma_f32(ptr(x), ptr(g), ptr(out), ptr(mx), ptr(stats), B, H, T, W, C, st, rt, ss, rs, flags,
                                            ptr(res), ws, wsb, stream_of(out)), "smooth_aniso_dsigma")
    return res


def _sigma_value(sigma):
    return float(sigma.detach()) if isinstance(sigma, torch.Tensor) else float(sigma)


def _aniso_forward(ctx, x, sigma_t, sigma_s, radius_t, radius_s, flags, group, sharded):
    cfg = (_sigma_value(sigma_t), radius_t, _sigma_value(sigma_s), radius_s, flags)
    out, mx = _aniso_fwd(x, cfg, group, sharded)
    learn = [isinstance(s, torch.Tensor) and s.requires_grad for s in (sigma_t, sigma_s)]
    ctx.save_for_backward(x if any(learn) else None, out, mx)
    ctx.cfg, ctx.group, ctx.sharded = cfg, group, sharded
    ctx.like = [s if l else None for s, l in zip((sigma_t, sigma_s), learn)]
    return out


def _aniso_backward(ctx, g):
    """(din, d sigma_t, d sigma_s): only what was asked for is computed"""
    x, out, mx = ctx.saved_tensors
    g = g.contiguous()
    want_din = ctx.needs_input_grad[0]
    want_sig = [ctx.needs_input_grad[1 + i] and ctx.like[i] is not None for i in (0, 1)]
    din, stats = None, None
    if ctx.sharded:
        din, stats = _aniso_bwd_sharded(g, out, mx, ctx.cfg, ctx.group, want_din)
    elif want_din:
        din = _aniso_bwd(g, out, mx, ctx.cfg)
    ds = [None, None]
    if any(want_sig):
        res = _aniso_dsigma(x, g, out, mx, stats, ctx.cfg)
        for i in (0, 1):
            if want_sig[i]:
                like = ctx.like[i]
                ds[i] = res[i].reshape(like.shape).to(device=like.device, dtype=like.dtype)
    return din, ds[0], ds[1]


class _SmoothAniso(torch.autograd.Function):
    """The anisotropic 3-D smoothing (include/kccot_smooth_aniso.h).  NOT reference behaviour.  ``sigma_t`` / ``sigma_s``: a
    float (a constant of the call) or a one-element tensor that requires a gradient (learnable); the value of a tensor is
    read on the host (a synchronisation when it lives on the device), so the learnable path can NOT be captured into a
    hipGraph.  out and din come from the same entry points, and are the same bits, whether or not a sigma is learnable.
    d loss / d sigma by kccot_smooth_aniso_dsigma_f32, in the sigma's shape, dtype and device; only the requested
    gradients are computed.  Once differentiable."""

    @staticmethod
    def forward(ctx, x, sigma_t, sigma_s, radius_t, radius_s, flags):
        return _aniso_forward(ctx, x, sigma_t, sigma_s, radius_t, radius_s, flags, None, False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _aniso_backward(ctx, g) + (None, None, None)


class _SmoothAnisoSharded(torch.autograd.Function):
    """_SmoothAniso for a batch that is sharded over the ranks of ``group`` (see _SmoothSharded): the forward is NO_DIVIDE ->
    all-reduce(MAX) -> EXTERNAL_MAX, the backward STATS_ONLY -> all-reduce(SUM) -> EXTERNAL_STATS.  The values returned for
    learnable sigmas are this rank's PARTIALS of d loss / d sigma (the GLOBAL maximum and sums over this rank's shard), the
    convention of _SmoothShardedSigma: nothing is all-reduced for them here."""

    @staticmethod
    def forward(ctx, x, sigma_t, sigma_s, radius_t, radius_s, flags, group):
        return _aniso_forward(ctx, x, sigma_t, sigma_s, radius_t, radius_s, flags, group, True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        return _aniso_backward(ctx, g) + (None, None, None, None)


def _all_reduce(t, op, group):
    import torch.distributed as dist
    if dist.get_backend(group) == "gloo" and t.is_cuda:       # CPU rehearsal backend: staged through the host
        h = t.cpu()
        dist.all_reduce(h, op=op, group=group)
        t.copy_(h)
    else:
        dist.all_reduce(t, op=op, group=group)


def _video(x):
    if x.dim() != 5:
        raise ValueError("expected a [B,H,T,W,C] video tensor, got shape %s" % (tuple(x.shape),))
    _lib.require_gpu(x)
    x = x if x.dtype == torch.float32 else x.float()
    return x.contiguous()


class KernelSmoothing:
    """data_utils.py:478-586.  Same constructor and method names as the reference."""

    def __init__(self, temporal_kernel_size=6, spatial_kernel_size=8, group=None, sharded=False):
        """``sharded=True`` (or a ``group``): the inputs are this rank's shard of a batch spread over the ranks of
        ``group`` (default group if None); the global maximum and its adjoint are all-reduced (_SmoothSharded)."""
        self.temporal_radius = temporal_kernel_size // 2   # data_utils.py:480
        self.spatial_radius = spatial_kernel_size // 2     # data_utils.py:481
        self.group, self.sharded = group, bool(sharded or group is not None)

    def _apply(self, inputs, sigma, radius, axes):
        """A float sigma, or a tensor that does not require a gradient, is a constant of the call.  A one-element tensor
        that requires a gradient is learnable: _SmoothSigma / _SmoothShardedSigma return its gradient as well."""
        if isinstance(sigma, torch.Tensor) and sigma.requires_grad:
            if sigma.numel() != 1 or not sigma.is_floating_point():
                raise ValueError("a learnable sigma is a 0-dim or one-element float tensor, got %s of shape %s"
                                 % (sigma.dtype, tuple(sigma.shape)))
            if self.sharded:
                return _SmoothShardedSigma.apply(_video(inputs), sigma, radius, axes, self.group)
            return _SmoothSigma.apply(_video(inputs), sigma, radius, axes)
        if self.sharded:
            return _SmoothSharded.apply(_video(inputs), float(sigma), radius, axes, self.group)
        return _Smooth.apply(_video(inputs), float(sigma), radius, axes)

    def gaussian_kernel1d(self, radius, sigma):
        """data_utils.py:483-491 (host-side helper; the kernels compute the same taps)."""
        x = torch.arange(-radius, radius + 1, dtype=torch.float32)
        k = torch.exp(torch.tensor(-0.5 / (sigma * sigma), dtype=torch.float32) * x ** 2)
        return k / k.sum()

    def gaussian_kernel3d(self, radius, sigma):
        """data_utils.py:493-501: shape [2r+1, 2r+1, 2r+1, 1, 1], normalised."""
        x = torch.arange(-radius, radius + 1, dtype=torch.float32)
        xx, yy, zz = torch.meshgrid(x, x, x, indexing="xy")
        k = torch.exp(torch.tensor(-0.5 / (sigma * sigma), dtype=torch.float32) * (xx ** 2 + yy ** 2 + zz ** 2))
        return (k / k.sum())[:, :, :, None, None]

    def temporal_convolution(self, inputs, sigma):
        """data_utils.py:503-521: 1-D Gaussian along T (REFLECT), then / global max."""
        return self._apply(inputs, sigma, self.temporal_radius, _lib.SMOOTH_T)

    def causal_temporal_convolution(self, inputs, sigma):
        """NOT reference behaviour.  The reference's only temporal smoothing is the symmetric stencil above, whose frame t
        contains frames t+1 .. t+r: features that are meant to depend on frames <= t see the future through it.  This is
        the past-only counterpart (KCCOT_SMOOTH_CAUSAL_T in include/kccot.h): with w_d = exp(-d^2 / (2 sigma^2)),
        s[t] = sum_{d=0}^{min(r,t)} w_d x[t-d] / sum_{d=0}^{min(r,t)} w_d -- no padding, the early frames use the truncated,
        renormalised window, so s[0] = x[0] -- then / global max.  Radius: the temporal one."""
        return self._apply(inputs, sigma, self.temporal_radius, _lib.SMOOTH_T | _lib.SMOOTH_CAUSAL_T)

    def spatial_convolution(self, inputs, sigma):
        """NOT reference behaviour.  The reference's 2-D path (data_utils.py:523-550) convolves
        VALID without padding and then reshapes the shrunken result to the input shape, which
        raises for every input; there is nothing to be compatible with.  Provided as the
        consistent extension: 2-D Gaussian over (H, W) with REFLECT borders, then / global max."""
        return self._apply(inputs, sigma, self.spatial_radius, _lib.SMOOTH_H | _lib.SMOOTH_W)

    def gaussian_convolution3D(self, inputs, sigma):
        """data_utils.py:552-582: 3-D Gaussian over (T, H, W), all with the SPATIAL radius
        (data_utils.py:553,562-564), REFLECT borders, then / global max."""
        return self._apply(inputs, sigma, self.spatial_radius, _lib.SMOOTH_T | _lib.SMOOTH_H | _lib.SMOOTH_W)

    def causal_gaussian_convolution3D(self, inputs, sigma):
        """NOT reference behaviour.  gaussian_convolution3D above smooths symmetrically along T too, so frame t of its
        output contains frames t+1 .. t+r.  This is its causal form (include/kccot_smooth_causal3.h): along T the past-only
        stencil of causal_temporal_convolution (truncated, renormalised window, no padding, s[0] = x[0]), along W and H the
        symmetric Gaussian with REFLECT borders, then / global max.  All three axes use the SPATIAL radius, as
        gaussian_convolution3D does."""
        return self._apply(inputs, sigma, self.spatial_radius, CAUSAL3)

    def anisotropic_gaussian_convolution3D(self, inputs, sigma_t, sigma_s, causal=False):
        """NOT reference behaviour.  The 3-D smoothing with SEPARATE bandwidths and radii for time and space
        (include/kccot_smooth_aniso.h): along T the Gaussian of ``sigma_t`` with the TEMPORAL radius -- unlike
        gaussian_convolution3D and causal_gaussian_convolution3D, which use the spatial radius on T as the reference does --
        and along H and W the Gaussian of ``sigma_s`` with the spatial radius, REFLECT borders, then / global max.
        ``causal=True``: along T the past-only stencil of causal_temporal_convolution instead (truncated, renormalised
        window, no padding, s[0] = x[0]).  A radius of 0 makes that axis group the identity.
        Each sigma is a float, a tensor that does not require a gradient (both constants of the call), or a one-element
        float tensor that requires a gradient (learnable: its gradient is returned as well); either, both or neither."""
        for name, s in (("sigma_t", sigma_t), ("sigma_s", sigma_s)):
            if isinstance(s, torch.Tensor) and s.requires_grad and (s.numel() != 1 or not s.is_floating_point()):
                raise ValueError("a learnable %s is a 0-dim or one-element float tensor, got %s of shape %s"
                                 % (name, s.dtype, tuple(s.shape)))
        sigma_t, sigma_s = (s if isinstance(s, torch.Tensor) and s.requires_grad else float(s) for s in (sigma_t, sigma_s))
        flags = _lib.SMOOTH_CAUSAL_T if causal else 0
        if self.sharded:
            return _SmoothAnisoSharded.apply(_video(inputs), sigma_t, sigma_s, self.temporal_radius, self.spatial_radius, flags,
                                             self.group)
        return _SmoothAniso.apply(_video(inputs), sigma_t, sigma_s, self.temporal_radius, self.spatial_radius, flags)

    def annealing_sigma(self, init_sigma, step, decay_steps=500, decay_rate=0.975):
        """data_utils.py:584-586."""
        return init_sigma * decay_rate ** (step / decay_steps)
