"""Torch flavour of the KernelSmoothing oracle (autograd gives the gradient oracle, including
the arg-max path of the global-max normalisation).  TEST INFRASTRUCTURE ONLY; pinned against
oracle/smoothing_np.py in tests/test_oracle_smoothing.py.  Runs on any device and in any float
dtype: the GPU tests evaluate it in float64 on the device, next to the kernels."""
import torch


def gaussian_kernel1d(radius, sigma, dtype=torch.float32, device=None):
    x = torch.arange(-radius, radius + 1, dtype=dtype, device=device)
    k = torch.exp(torch.tensor(-0.5 / (sigma * sigma), dtype=dtype, device=device) * x ** 2)
    return k / k.sum()


def _reflect_index(n, r, device=None):
    idx = torch.arange(-r, n + r, device=device)
    idx = torch.where(idx < 0, -idx, idx)
    return torch.where(idx >= n, 2 * (n - 1) - idx, idx)


def conv_axis(v, w, axis):
    r = (len(w) - 1) // 2
    n = v.shape[axis]
    vp = v.index_select(axis, _reflect_index(n, r, v.device))
    out = 0
    for d in range(2 * r + 1):
        out = out + w[d] * vp.narrow(axis, d, n)
    return out


def smooth(v, sigma, radius, axes, normalise=True):
    """v: [B,H,T,W,C]; axes: subset of (2, 1, 3) = (T, H, W)."""
    w = gaussian_kernel1d(radius, sigma, v.dtype, v.device)
    s = v
    for a in axes:
        s = conv_axis(s, w, a)
    return s / s.max() if normalise else s


def smooth_transpose(u, sigma, radius, axes):
    """A^T u, A = the unnormalised smoothing (linear, REFLECT borders folded back): torch autograd of
    ``smooth(..., normalise=False)`` in u's dtype.  A does not couple samples, so any batch slab of u
    gives the same slab of A^T u."""
    x = torch.zeros_like(u, requires_grad=True)
    with torch.enable_grad():
        s = smooth(x, sigma, radius, axes, normalise=False)
        (g,) = torch.autograd.grad(s, x, u)
    return g


def maxnorm_stats(gout, out):
    """The two batch sums of the normalisation's adjoint: (sum gout * out in fp64, number of out == 1)."""
    return float((gout.double() * out.double()).sum()), int((out == 1).sum())


def smooth_bwd(gout, out, mx, sigma, radius, axes, stats=None, slab=None, dtype=torch.float64):
    """Adjoint of out = s / max(s), s = A x, for the operation the kernels compute, from the KERNEL'S OWN forward output
    ``out`` and maximum ``mx``:

        din = A^T (gout / max - corr [out == 1]),   corr = sum(gout * out) / (max * n_ties)

    (the reference divides by reduce_max, whose gradient splits evenly over all exact ties).  ``stats``: the global
    (sum gout * out, n_ties) when ``gout`` / ``out`` are one shard of a larger batch; default: this tensor's own
    (maxnorm_stats).  ``slab``: samples per A^T evaluation, which bounds the memory of the ``dtype`` intermediates."""
    dot, ties = maxnorm_stats(gout, out) if stats is None else stats
    m = float(mx)
    corr = dot / (m * ties) if ties else 0.0
    B = out.shape[0]
    slab = slab or B
    din = torch.empty(out.shape, dtype=dtype, device=out.device)
    for b0 in range(0, B, slab):
        u = gout[b0:b0 + slab].to(dtype) / m
        if ties:
            u -= corr * (out[b0:b0 + slab] == 1).to(dtype)
        din[b0:b0 + slab] = smooth_transpose(u, sigma, radius, axes)
        del u
    return din
