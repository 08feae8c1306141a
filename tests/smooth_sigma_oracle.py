"""fp64 oracle of d loss / d sigma of the kernel smoothing (include/kccot_smooth_sigma.h), in torch on any device.  A helper of
tests/test_smooth_sigma_cpu.py (which validates it against finite differences) and tests/test_gpu_smooth_sigma.py.

Forms: "T", "causalT", "HW", "THW", "causalTHW" on [B,H,T,W,C] tensors; stage order T, W, H."""
import math

import numpy as np
import torch

FORMS = ("T", "causalT", "HW", "THW", "causalTHW")
_AXES = {"T": (2,), "causalT": (2,), "HW": (3, 1), "THW": (2, 3, 1), "causalTHW": (2, 3, 1)}     # dims of [B,H,T,W,C]


def flags(form):
    """axes_flags of kccot_smooth_dsigma_f32"""
    return {"T": 1, "causalT": 1 | 8, "HW": 2 | 4, "THW": 1 | 2 | 4, "causalTHW": 1 | 2 | 4 | 8}[form]


def _round32(t):
    return t.to(torch.float32).to(torch.float64)


def sym_taps(sigma, r, round32=False):
    """(w, w') for d = -r..r from the fp64 number `sigma`; round32: the taps the kernel is handed (rounded to fp32)"""
    d = torch.arange(-r, r + 1, dtype=torch.float64)
    e = torch.exp(-d * d / (2.0 * sigma * sigma))
    w = e / e.sum()
    mu2 = (w * d * d).sum()
    dw = w * (d * d - mu2) / sigma ** 3
    return (_round32(w), _round32(dw)) if round32 else (w, dw)


def causal_taps(sigma, r, T, round32=False):
    """(V, V') of shape [T, r+1]: row t holds v_{t,d}, d = 0..min(r,t), zeros behind"""
    d = torch.arange(0, r + 1, dtype=torch.float64)
    e = torch.exp(-d * d / (2.0 * sigma * sigma))
    t = torch.arange(T, dtype=torch.float64)[:, None]
    live = (d[None, :] <= t).to(torch.float64)
    V = e[None, :] * live
    V = V / V.sum(1, keepdim=True)
    mu2 = (V * d * d).sum(1, keepdim=True)
    dV = V * (d * d - mu2) / sigma ** 3
    return (_round32(V), _round32(dV)) if round32 else (V, dV)


def _sym(x, k, dim):
    """REFLECT stencil along `dim` with taps k[d + r]"""
    L, r = x.shape[dim], (k.numel() - 1) // 2
    p = torch.arange(L, device=x.device)
    out = torch.zeros_like(x)
    for d in range(-r, r + 1):
        q = (p + d).abs()
        q = torch.where(q >= L, 2 * (L - 1) - q, q)
        out = out + float(k[d + r]) * x.index_select(dim, q)
    return out


def _causal(x, V, dim):
    """out[t] = sum_d V[t, d] x[t - d] (no padding: V is zero where t - d < 0)"""
    L, r = x.shape[dim], V.shape[1] - 1
    p = torch.arange(L, device=x.device)
    shape = [1] * x.dim()
    shape[dim] = L
    out = torch.zeros_like(x)
    for d in range(0, r + 1):
        out = out + V[:, d].to(x.device).reshape(shape) * x.index_select(dim, (p - d).clamp(min=0))
    return out


def fields(x, sigma, r, form, absolute=False, round32=False):
    """(s, ds/dsigma) in fp64: s = A x, ds/dsigma = sum_a (prod_{b != a} A_b) A'_a x.  absolute: the yardstick operator,
    the same sum with |w'|, w and |x| (s is then A |x|)."""
    F = x.to(torch.float64)
    if absolute:
        F = F.abs()
    G = torch.zeros_like(F)
    w, dw = sym_taps(sigma, r, round32)
    if absolute:
        dw = dw.abs()
    for dim in _AXES[form]:
        if dim == 2 and form.startswith("causal"):
            V, dV = causal_taps(sigma, r, x.shape[2], round32)
            if absolute:
                dV = dV.abs()
            F, G = _causal(F, V, dim), _causal(F, dV, dim) + _causal(G, V, dim)
        else:
            F, G = _sym(F, w, dim), _sym(F, dw, dim) + _sym(G, w, dim)
    return F, G


def upstream(g, out, mx, stats=None):
    """u = g / m - [out == 1] (sum g*out) / (m n_ties) in fp64, from the forward's own out and maximum"""
    g, out, m = g.to(torch.float64), out.to(torch.float64), float(mx)
    tie = out == 1.0
    dot, nt = ((g * out).sum(), tie.sum()) if stats is None else (stats[0], stats[1])
    dot, nt = float(dot), float(nt)         # (Python floats: an int64 count times a float would promote to fp32)
    u = g / m
    if nt > 0:
        u = u - tie.to(torch.float64) * (dot / (m * nt))
    return u


def dsigma_ref(x, g, out, mx, sigma, r, form, stats=None, round32=True):
    """(dsigma_ref, Y): dsigma_ref = sum u * ds/dsigma and the yardstick Y = sum |u| * (|A'| |x|)"""
    u = upstream(g, out, mx, stats)
    _, ds = fields(x, sigma, r, form, False, round32)
    _, ya = fields(x, sigma, r, form, True, round32)
    return float((u * ds).sum()), float((u.abs() * ya).sum())


def loss64(x, g, sigma, r, form):
    """sum g * (s / max s) in fp64: what the finite difference differentiates"""
    s, _ = fields(x, sigma, r, form)
    return float((g.to(torch.float64) * s / s.max()).sum())


def f32(v):
    return float(np.float32(v))


def all_offdiagonal_taps_underflow(sigma, r):
    """True where the kernel's derivative taps are all zero (every e_d, d != 0, is below fp32 after the division by sigma^3)"""
    _, dw = sym_taps(f32(sigma), max(r, 1), round32=True)
    return bool((dw == 0).all()) and math.exp(-1.0 / (2.0 * f32(sigma) ** 2)) < 1e-45
