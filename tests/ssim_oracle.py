"""The definition of include/kccot_metrics.h transcribed in torch: the SSIM map, the per-frame scores, the mean squared error and
the closed-form adjoint with respect to y.  Not a test module: tests/test_ssim_cpu.py checks it against autograd and scipy, and
tests/test_gpu_ssim.py runs it in fp64 on the device as the reference of the kernels.  Everything runs on the device and in the
dtype of its inputs; only the taps are always this library's fp32 taps (csrc/smooth_internal.h, make_taps)."""
import numpy as np
import torch

# (B,H,T,W,C), win_size, sigma, input builder: the grid of the GPU tests and of the CPU test of the reference's own fp32 error.
# The kernels cut a row into column tiles once (columns x channels) passes 256 positions and into channel tiles past 16 channels:
# the last two rows are there for that.
GRID = [
    ((2, 8, 3, 9, 1), 3, 1.5, "noise"),         # the smallest case
    ((1, 11, 2, 11, 1), 11, 1.5, "noise"),      # a 1 x 1 map: H = W = 2r + 1
    ((1, 13, 2, 70, 3), 11, 1.5, "noise"),      # C = 3 strides, positions left idle in the last wave (one column tile: 210 <= 256)
    ((1, 70, 2, 13, 2), 11, 1.5, "noise"),      # more than one segment of the H walk
    ((2, 16, 4, 16, 2), 15, 0.5, "noise"),      # the maximal radius, taps that underflow to 0
    ((3, 9, 5, 10, 1), 1, 1.5, "noise"),        # r = 0
    ((2, 64, 5, 64, 1), 11, 1.5, "noise"),      # the workload's frame at a small T
    ((1, 23, 3, 11, 1), 11, 1.5, "flat"),       # cancellation in G(x^2) - mx^2
    ((1, 13, 2, 100, 3), 11, 1.5, "noise"),     # two column tiles both ways (forward 85 + 5 map columns, backward 75 + 25 of dy)
    ((1, 12, 2, 20, 20), 3, 1.5, "noise"),      # two channel tiles (16 + 4 of 20) times two column tiles both ways
]
CAP_SSIM = {"noise": 1e-5, "flat": 5e-5}        # |ssim - ref|
CAP_DY = 1e-4                                   # |dy - ref| / max|ref|, noise only
CAP_MSE = 2e-6                                  # |mse - ref| / ref


def taps(sigma, r):
    """make_taps: e_d = exp(coef d^2) in fp32 with coef = fp32(-0.5 / sigma^2) from the fp32 value of sigma, summed in fp32 in
    ascending d, each divided by the sum.  Returned as float64 holding the fp32 values."""
    s = float(np.float32(sigma))
    coef = np.float32(-0.5 / (s * s))
    e = [np.exp(np.float32(coef * np.float32(d * d)), dtype=np.float32) for d in range(-r, r + 1)]
    tot = np.float32(0.0)
    for v in e:
        tot = np.float32(tot + v)
    return torch.tensor([float(np.float32(v / tot)) for v in e], dtype=torch.float64)


def _corr(v, w, dim):
    """VALID correlation along `dim`: out[i] = sum_a w_a v[i + a], added up in ascending a"""
    n = v.shape[dim] - (len(w) - 1)
    out = None
    for a in range(len(w)):
        term = w[a] * v.narrow(dim, a, n)
        out = term if out is None else out + term
    return out


def gauss(v, w):
    """G v on [B,H,T,W,C]: W then H"""
    w = w.to(v.device, v.dtype)
    return _corr(_corr(v, w, 3), w, 1)


def gauss_t(m, w):
    """G^T m: the full correlation of a [B,H-2r,T,W-2r,C] map back onto H x W"""
    r2 = len(w) - 1
    w = w.to(m.device, m.dtype).flip(0)
    p = torch.nn.functional.pad(m, (0, 0, r2, r2, 0, 0, r2, r2))       # (C, W, T, H from the last dimension backwards)
    return _corr(_corr(p, w, 3), w, 1)


def _terms(x, y, sigma, r, L):
    w = taps(sigma, r)
    mx, my = gauss(x, w), gauss(y, w)
    sxx, syy, sxy = gauss(x * x, w) - mx * mx, gauss(y * y, w) - my * my, gauss(x * y, w) - mx * my
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    A1, A2, B1, B2 = 2 * mx * my + c1, 2 * sxy + c2, mx * mx + my * my + c1, sxx + syy + c2
    return w, mx, my, A1, A2, B1, B2


def ssim_map(x, y, sigma, r, L=1.0):
    """S [B,H-2r,T,W-2r,C]"""
    _, _, _, A1, A2, B1, B2 = _terms(x, y, sigma, r, L)
    return A1 * A2 / (B1 * B2)


def scores(x, y, sigma, r, L=1.0):
    """ssim [B,T]"""
    return ssim_map(x, y, sigma, r, L).mean(dim=(1, 3, 4))


def mse(x, y):
    """[B,T]"""
    return ((x - y) ** 2).mean(dim=(1, 3, 4))


def adjoint(g, x, y, sigma, r, L=1.0):
    """dy of sum_bt g[b,t] ssim[b,t] from the closed form of the header"""
    w, mx, my, A1, A2, B1, B2 = _terms(x, y, sigma, r, L)
    S = A1 * A2 / (B1 * B2)
    B, Hm, T, Wm, C = S.shape
    u = (g.to(S.dtype) / (Hm * Wm * C))[:, None, :, None, None]
    alpha = -S / B2
    beta = 2 * A1 / (B1 * B2)
    gamma = 2 * mx * A2 / (B1 * B2) - 2 * my * S / B1 - beta * mx - 2 * alpha * my
    return gauss_t(u * gamma, w) + 2 * y * gauss_t(u * alpha, w) + x * gauss_t(u * beta, w)


def noise(shape, seed, device="cpu"):
    """x = rand, y = clamp(x + 0.1 randn, 0, 1), float32"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen)
    y = (x + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1)
    return x.to(device), y.to(device)


def flat(shape, seed, device="cpu"):
    """the bright, nearly constant case: x = 0.95 + 0.01 rand, y = clamp(x + 0.1 randn, 0, 1), float32"""
    gen = torch.Generator().manual_seed(seed)
    x = 0.95 + 0.01 * torch.rand(shape, generator=gen)
    y = (x + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1)
    return x.to(device), y.to(device)


def inputs(kind, shape, seed, device="cpu"):
    return {"noise": noise, "flat": flat}[kind](shape, seed, device)


def upstream(shape, seed, device="cpu"):
    """g [B,T], float32"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((shape[0], shape[2]), generator=gen).to(device)
