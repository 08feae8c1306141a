"""fp64 oracle of the anisotropic 3-D kernel smoothing (include/kccot_smooth_aniso.h), in torch on any device: the forward, the
adjoint through the header's effective border taps, and the two bandwidth gradients.  Built from the stencils of
tests/smooth_sigma_oracle.py.  A helper of tests/test_aniso_smoothing_cpu.py (which validates it against finite differences and
autograd) and tests/test_gpu_aniso_smoothing.py.

[B,H,T,W,C] tensors; stage order T, W, H; a radius of 0 makes its axis group the identity."""
import torch

from smooth_sigma_oracle import sym_taps, causal_taps, _sym, _causal, upstream, f32  # noqa: F401  (re-exported)

CAUSAL_T, NO_DIVIDE, EXTERNAL_MAX, STATS_ONLY, EXTERNAL_STATS = 8, 16, 32, 64, 128


def _t_taps(sigma_t, rt, T, causal, round32):
    return causal_taps(sigma_t, rt, T, round32) if causal else sym_taps(sigma_t, rt, round32)


def _t_apply(x, k, causal):
    return _causal(x, k, 2) if causal else _sym(x, k, 2)


def fields(x, sigma_t, sigma_s, rt, rs, causal, absolute=False, round32=False):
    """(s, ds/dsigma_t, ds/dsigma_s) in fp64.  absolute: the yardstick operators, the same sums with |w'|, w and |x|."""
    F = x.to(torch.float64)
    if absolute:
        F = F.abs()
    Gt, Gs = torch.zeros_like(F), torch.zeros_like(F)
    if rt > 0:
        k, dk = _t_taps(sigma_t, rt, x.shape[2], causal, round32)
        if absolute:
            dk = dk.abs()
        F, Gt = _t_apply(F, k, causal), _t_apply(F, dk, causal)
    if rs > 0:
        w, dw = sym_taps(sigma_s, rs, round32)
        if absolute:
            dw = dw.abs()
        for dim in (3, 1):
            F, Gt, Gs = _sym(F, w, dim), _sym(Gt, w, dim), _sym(F, dw, dim) + _sym(Gs, w, dim)
    return F, Gt, Gs


def forward(x, sigma_t, sigma_s, rt, rs, causal):
    """(out, m, s)"""
    s = fields(x, sigma_t, sigma_s, rt, rs, causal)[0]
    m = s.max()
    return s / m, m, s


def reflect_adjoint_matrix(k, L):
    """M[p, q] = the coefficient of u[q] in din[p] for the REFLECT stencil with taps k[d + r] on an axis of length L > r:
    w[q-p] + [p >= 1 and p+q <= r] w[p+q] + [p <= L-2 and (L-1-p)+(L-1-q) <= r] w[2(L-1)-p-q] over |q - p| <= r."""
    r = (k.numel() - 1) // 2
    M = torch.zeros((L, L), dtype=torch.float64)
    for p in range(L):
        for q in range(max(0, p - r), min(L, p + r + 1)):
            c = float(k[q - p + r])
            if p >= 1 and p + q <= r:
                c += float(k[p + q + r])
            if p <= L - 2 and (L - 1 - p) + (L - 1 - q) <= r:
                c += float(k[2 * (L - 1) - p - q + r])
            M[p, q] = c
    return M


def causal_adjoint_matrix(V):
    """M[p, p+d] = v_{p+d,d}: din[p] = sum_{d=0..r, p+d<T} v_{p+d,d} u[p+d]"""
    T, r = V.shape[0], V.shape[1] - 1
    M = torch.zeros((T, T), dtype=torch.float64)
    for p in range(T):
        for d in range(0, r + 1):
            if p + d < T:
                M[p, p + d] = float(V[p + d, d])
    return M


def _apply_matrix(M, u, dim):
    return torch.tensordot(M.to(u.device), u.movedim(dim, 0), dims=1).movedim(0, dim)


def adjoint(u, sigma_t, sigma_s, rt, rs, causal):
    """din = A_t^T A_w^T A_h^T u as gathers with the effective taps (T, W, H order: the operators commute)"""
    d = u.to(torch.float64)
    if rt > 0:
        k = _t_taps(sigma_t, rt, u.shape[2], causal, False)[0]
        d = _apply_matrix(causal_adjoint_matrix(k) if causal else reflect_adjoint_matrix(k, u.shape[2]), d, 2)
    if rs > 0:
        w = sym_taps(sigma_s, rs)[0]
        for dim in (3, 1):
            d = _apply_matrix(reflect_adjoint_matrix(w, u.shape[dim]), d, dim)
    return d


def dsigma_ref(x, g, out, mx, sigma_t, sigma_s, rt, rs, causal, stats=None, round32=True):
    """((dsigma_t, dsigma_s), (Y_t, Y_s)): Y_t = sum |u| (|A_h| |A_w| |A'_t| |x|), Y_s analogously"""
    u = upstream(g, out, mx, stats)
    _, gt, gs = fields(x, sigma_t, sigma_s, rt, rs, causal, False, round32)
    _, yt, ys = fields(x, sigma_t, sigma_s, rt, rs, causal, True, round32)
    return (float((u * gt).sum()), float((u * gs).sum())), (float((u.abs() * yt).sum()), float((u.abs() * ys).sum()))


def loss64(x, g, sigma_t, sigma_s, rt, rs, causal):
    """sum g * (s / max s) in fp64: what the finite differences differentiate"""
    s = fields(x, sigma_t, sigma_s, rt, rs, causal)[0]
    return float((g.to(torch.float64) * s / s.max()).sum())
