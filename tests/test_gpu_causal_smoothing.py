"""KCCOT_SMOOTH_CAUSAL_T, the past-only temporal smoothing (NOT reference behaviour: the specification is include/kccot.h), on
guarded buffers (tests/abi_guard.py) against a float64 oracle written out below.

    s[t] = sum_{d=0}^{min(r,t)} w_d x[t-d] / sum_{d=0}^{min(r,t)} w_d,   w_d = exp(-d^2 / (2 sigma^2)),   out = s / max(s)

Tolerances are the ones tests/test_gpu_smoothing_fp64.py holds the symmetric temporal call to (forward 1e-6 absolute, din 1e-5
of max|din_ref|): the chain here is r + 1 <= 2r + 1 terms of the same arithmetic.  The gradient reference is autograd through
the oracle; torch's amax splits the gradient evenly over tied maxima, which is the library's convention
(corr = sum(g * out) / (max * #ties) at every element with out == 1, tests/test_gpu_smoothing_fp64.py).

Shapes: (2,4,9,8,1) float4 pieces; (1,3,5,5,3) W*C = 15, single floats; (1,2,2,4,1) radius >= T; (1,2,1,4,1) T = 1;
(3,8,30,16,1) the configs[1] T; and (4,50,1,101,1), where a folded backward would need more tie records than the workspace
holds and must take the two-pass form."""
import pytest
import torch

import abi_guard as ag

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SHAPES = [(2, 4, 9, 8, 1), (1, 3, 5, 5, 3), (1, 2, 2, 4, 1), (1, 2, 1, 4, 1), (3, 8, 30, 16, 1)]
SIGMAS = (5.0, 1.3, 0.03)
RADII = (3, 4, 6, 0)
ATOL_FWD, DIN_TOL = 1e-6, 1e-5


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


def oracle(x, sigma, r, normalise=True):
    """fp64, on the CPU: the definition, term by term."""
    x = x.double()
    T = x.shape[2]
    w = torch.exp(-torch.arange(r + 1, dtype=F64) ** 2 / (2.0 * sigma * sigma))
    s = torch.zeros_like(x)
    for d in range(min(r, T - 1) + 1):
        s[:, :, d:] = s[:, :, d:] + w[d] * x[:, :, :T - d]
    Z = torch.cumsum(w, 0)[torch.arange(T).clamp(max=r)]
    s = s / Z.view(1, 1, T, 1, 1)
    return s / s.amax() if normalise else s


def oracle_grad(x, g, sigma, r):
    xd = x.double().requires_grad_(True)
    out = oracle(xd, sigma, r)
    (out * g.double()).sum().backward()
    return out.detach(), xd.grad


def _verify(*bufs):
    torch.cuda.synchronize()
    bad = [m for m in (b.verify() for b in bufs) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)


def fwd(L, x, sigma, r, flags, mx=None, offset=0):
    """kccot_smooth_fwd_f32 on guarded buffers; returns (out, max) on the CPU."""
    shape = tuple(x.shape)
    gin = ag.guarded_input("in", x.cuda(), offset)
    gout = ag.guarded(x.numel() * 4, "output", "out", offset)
    gmx = ag.guarded(4, "output", "max_inout")
    if mx is not None:
        gmx.view(F32, (1,)).copy_(mx)
    gws = ag.guarded(int(L.lib.kccot_smooth_workspace_bytes(*shape)), "workspace", "ws")
    rc = L.lib.kccot_smooth_fwd_f32(gin.ptr, *shape, sigma, r, flags, gout.ptr, gmx.ptr, gws.ptr, gws.nbytes, None)
    assert rc == 0, L.lib.kccot_last_error()
    _verify(gin, gout, gmx, gws)
    assert torch.equal(gin.view(F32, shape).cpu(), x.cpu()), "the input was written"
    return gout.view(F32, shape).cpu(), gmx.view(F32, (1,)).cpu()


def bwd(L, g, out, mx, sigma, r, flags, stats=None, offset=0):
    """kccot_smooth_bwd_f32, or the sharded entry point: stats == "only" returns the two sums, a tensor is handed in."""
    shape = tuple(out.shape)
    gg, go = ag.guarded_input("gout", g.cuda(), offset), ag.guarded_input("out", out.cuda(), offset)
    gmx = ag.guarded_input("max_in", mx.cuda())
    gdin = ag.guarded(out.numel() * 4, "output", "din", offset)
    gws = ag.guarded(int(L.lib.kccot_smooth_workspace_bytes(*shape)), "workspace", "ws")
    if stats is None:
        rc = L.lib.kccot_smooth_bwd_f32(gg.ptr, go.ptr, gmx.ptr, *shape, sigma, r, flags, gdin.ptr, gws.ptr, gws.nbytes, None)
        gst = gmx
    else:
        only = isinstance(stats, str)
        gst = ag.guarded(8, "output", "stats_inout") if only else ag.guarded_input("stats_inout", stats.cuda())
        rc = L.lib.kccot_smooth_bwd_sharded_f32(gg.ptr, go.ptr, gmx.ptr, gst.ptr, *shape, sigma, r,
                                                flags | (L.SMOOTH_STATS_ONLY if only else L.SMOOTH_EXTERNAL_STATS), gdin.ptr,
                                                gws.ptr, gws.nbytes, None)
    assert rc == 0, L.lib.kccot_last_error()
    _verify(gg, go, gmx, gdin, gws, gst)
    if stats is not None and isinstance(stats, str):
        assert bool(ag.unwritten(gdin.view(F32, shape)).all()), "STATS_ONLY wrote din"
        return gst.view(F32, (2,)).cpu()
    return gdin.view(F32, shape).cpu()


def _inputs(shape, seed):
    """A plain random video, and one whose maximum sits in an early frame (t < r: the truncated window and its own Z_t)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=gen)
    yield "random", x
    if shape[2] > 1:
        y = 0.5 * torch.rand(shape, generator=gen)
        y[0, 1, 1, 2, 0] = 3.0
        yield "early", y


@pytest.mark.parametrize("fold", [0, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_fp64(L, shape, fold):
    """Every sigma and radius (3 and 4 compiled in, 6 and 0 through the generic form), forward and adjoint, the two-pass
    backward (fold 0) and the folded one (fold 2: records, sparse fix-up, guarded dense walk); the float4 shape also from
    pointers that are only 4-byte aligned.  Canaries behind out, din, max_inout and the workspace are checked in every call."""
    flags = L.SMOOTH_T | L.SMOOTH_CAUSAL_T
    g = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    fails = []
    for kind, x in _inputs(shape, sum(shape)):
        for sigma in SIGMAS:
            for r in RADII:
                ref, din_ref = oracle_grad(x, g, sigma, r)
                for offset in ((0, 4) if shape == SHAPES[0] else (0,)):
                    with L.options(smooth_bwd_fold=fold):
                        out, mx = fwd(L, x, sigma, r, flags, offset=offset)
                        din = bwd(L, g, out, mx, sigma, r, flags, offset=offset)
                    e_fwd = float((out.double() - ref).abs().max())
                    e_din = float((din.double() - din_ref).abs().max()) / float(din_ref.abs().max())
                    tag = "%s %-6s sigma=%-4g r=%d offset=%d fold=%d" % (shape, kind, sigma, r, offset, fold)
                    print("%s: fwd %.2e  din %.2e  max(out) %r" % (tag, e_fwd, e_din, float(out.max())))
                    if float(out.max()) != 1.0:
                        fails.append("%s: max(out) = %r" % (tag, float(out.max())))
                    if not e_fwd <= ATOL_FWD:
                        fails.append("%s: forward %.3e > %.0e" % (tag, e_fwd, ATOL_FWD))
                    if not e_din <= DIN_TOL:
                        fails.append("%s: adjoint %.3e > %.0e" % (tag, e_din, DIN_TOL))
    assert not fails, "\n".join(fails)


def test_first_frame_is_the_input_and_a_constant_gives_ones(L):
    flags = L.SMOOTH_T | L.SMOOTH_CAUSAL_T
    x = torch.rand((2, 4, 9, 8, 1), generator=torch.Generator().manual_seed(5))
    raw, mx = fwd(L, x, 1.3, 3, flags | L.SMOOTH_NO_DIVIDE)
    assert torch.equal(raw[:, :, 0], x[:, :, 0]) and float(mx) == float(raw.max())
    ones, _ = fwd(L, torch.full((2, 4, 9, 8, 1), 0.37), 1.3, 3, flags)
    assert float((ones - 1.0).abs().max()) <= ATOL_FWD and float(ones.max()) == 1.0


def test_folded_backward_takes_the_two_pass_form_where_the_records_do_not_fit(L):
    """T = 1 and W*C = 101: single-float pieces, one frame per column, 79 workgroups -- the folded backward would lay 79 tie
    records where the workspace has room for 41, so smooth_bwd_fold = 2 runs the two-pass form (the workspace canary holds)."""
    flags = L.SMOOTH_T | L.SMOOTH_CAUSAL_T
    shape = (4, 50, 1, 101, 1)
    gen = torch.Generator().manual_seed(41)
    x, g = torch.rand(shape, generator=gen), torch.randn(shape, generator=gen)
    ref, din_ref = oracle_grad(x, g, 1.3, 3)
    with L.options(smooth_bwd_fold=2):
        out, mx = fwd(L, x, 1.3, 3, flags)
        din = bwd(L, g, out, mx, 1.3, 3, flags)
    assert float(out.max()) == 1.0 and float((out.double() - ref).abs().max()) <= ATOL_FWD
    assert float((din.double() - din_ref).abs().max()) <= DIN_TOL * float(din_ref.abs().max())


@pytest.mark.parametrize("shape,r", [((2, 4, 9, 8, 1), 3), ((1, 3, 9, 5, 3), 6)], ids=["float4_r3", "scalar_r6"])
def test_frames_up_to_t0_do_not_depend_on_later_frames(L, shape, r):
    """Causality itself: two videos that agree on frames <= t0 and differ after give bit-identical smoothed frames <= t0.  The
    symmetric stencil on the same pair does not, so the comparison can see a leak."""
    t0 = 4
    gen = torch.Generator().manual_seed(11)
    a = torch.rand(shape, generator=gen)
    b = a.clone()
    b[:, :, t0 + 1:] = torch.rand(b[:, :, t0 + 1:].shape, generator=gen)
    nd = L.SMOOTH_T | L.SMOOTH_NO_DIVIDE
    ca, _ = fwd(L, a, 1.3, r, nd | L.SMOOTH_CAUSAL_T)
    cb, _ = fwd(L, b, 1.3, r, nd | L.SMOOTH_CAUSAL_T)
    assert ag.same_bits(ca[:, :, :t0 + 1], cb[:, :, :t0 + 1])
    assert not torch.equal(ca[:, :, t0 + 1:], cb[:, :, t0 + 1:])
    sa, _ = fwd(L, a, 1.3, 3, nd)
    sb, _ = fwd(L, b, 1.3, 3, nd)
    assert not torch.equal(sa[:, :, :t0 + 1], sb[:, :, :t0 + 1]), "the symmetric stencil should leak frames > t0"


def _tied(n_ties):
    """n_ties identical voxels on a zero background: five next to each other along W in one row (one workgroup's record holds
    more than TIE_PER_WG = 4), the rest in columns of their own; all in frames t >= r, where Z_t is the same."""
    shape = (3, 8, 30, 16, 1)
    x = torch.zeros(shape)
    for w in range(5):
        x[0, 2, 10, w, 0] = 1.0
    rng = torch.Generator().manual_seed(n_ties)
    cols = torch.randperm(2 * 8 * 16, generator=rng)[:n_ties - 5]
    for i, c in enumerate(cols.tolist()):
        b, h, w = 1 + c // 128, (c // 16) % 8, c % 16
        x[b, h, 3 + (7 * i) % 27, w, 0] = 1.0
    assert int(x.sum()) == n_ties
    return x


@pytest.mark.parametrize("fold", [0, 2])
@pytest.mark.parametrize("n_ties", [5, 40])
def test_tied_maxima_share_the_correction(L, n_ties, fold):
    """5 tied maxima (the sparse fix-up's per-record limit exceeded) and 40 (above its 32 entries), two-pass and folded."""
    flags = L.SMOOTH_T | L.SMOOTH_CAUSAL_T
    x = _tied(n_ties)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
    for sigma in (1.3, 5.0):
        ref, din_ref = oracle_grad(x, g, sigma, 3)
        assert int((ref == 1).sum()) == n_ties
        with L.options(smooth_bwd_fold=fold):
            out, mx = fwd(L, x, sigma, 3, flags)
            din = bwd(L, g, out, mx, sigma, 3, flags)
            stats = bwd(L, g, out, mx, sigma, 3, flags, stats="only")
        assert torch.equal(out == 1, ref == 1) and int(stats[1]) == n_ties
        e_fwd = float((out.double() - ref).abs().max())
        e_din = float((din.double() - din_ref).abs().max()) / float(din_ref.abs().max())
        print("ties %d sigma %g fold %d: fwd %.2e din %.2e" % (n_ties, sigma, fold, e_fwd, e_din))
        assert e_fwd <= ATOL_FWD and e_din <= DIN_TOL


def test_sharded_protocol_on_one_gpu_equals_the_whole_batch(L):
    """The batch cut in two: NO_DIVIDE per half, the larger maximum, EXTERNAL_MAX; STATS_ONLY per half, the sums added,
    EXTERNAL_STATS.  Outputs and din equal the one call on the whole batch bit for bit.  A sample is 256 elements, one
    workgroup of the sums' first stage, so each half hands back ONE fp32 partial sum and the two add in a single rounding in
    either order -- with more partials per half the all-reduced fp32 sum and the one-call sum may differ in the last bit.
    One tied maximum in each half: the tie count is 1 + 1."""
    flags = L.SMOOTH_T | L.SMOOTH_CAUSAL_T
    shape, sigma, r = (2, 4, 8, 8, 1), 1.3, 3
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(shape, generator=gen)
    x[0, 1, 5, 2, 0] = x[1, 3, 5, 6, 0] = 4.0
    x[0, 1, 2:5, 2, 0] = x[1, 3, 2:5, 6, 0] = 0.25
    g = torch.randn(shape, generator=gen)
    with L.options(smooth_bwd_fold=0):
        one, m1 = fwd(L, x, sigma, r, flags)
        din1 = bwd(L, g, one, m1, sigma, r, flags)
        halves = [slice(0, 1), slice(1, 2)]
        maxima = [fwd(L, x[s], sigma, r, flags | L.SMOOTH_NO_DIVIDE)[1] for s in halves]
        mx = torch.maximum(*maxima)
        out = torch.cat([fwd(L, x[s], sigma, r, flags | L.SMOOTH_EXTERNAL_MAX, mx=mx)[0] for s in halves])
        assert ag.same_bits(mx, m1) and ag.same_bits(out, one)
        assert int((out == 1).sum()) == 2
        parts = [bwd(L, g[s], out[s], mx, sigma, r, flags, stats="only") for s in halves]
        stats = (parts[0].double() + parts[1].double()).float()
        assert int(stats[1]) == 2
        din = torch.cat([bwd(L, g[s], out[s], mx, sigma, r, flags, stats=stats) for s in halves])
    assert ag.same_bits(din, din1), float((din - din1).abs().max())
    _, din_ref = oracle_grad(x, g, sigma, r)
    assert float((din.double() - din_ref).abs().max()) <= DIN_TOL * float(din_ref.abs().max())


def test_argument_rules_leave_the_buffers_untouched(L):
    shape = (2, 4, 9, 8, 1)
    x = torch.rand(shape)
    gin, gout = ag.guarded_input("in", x.cuda()), ag.guarded(x.numel() * 4, "output", "out")
    gmx, gws = ag.guarded(4, "output", "max_inout"), ag.guarded(int(L.lib.kccot_smooth_workspace_bytes(*shape)), "workspace", "ws")
    before = [b.payload().clone() for b in (gout, gmx, gws)]
    Cz = L.SMOOTH_CAUSAL_T

    def call(flags, wsb=None, radius=3):
        return L.lib.kccot_smooth_fwd_f32(gin.ptr, *shape, 1.3, radius, flags, gout.ptr, gmx.ptr, gws.ptr,
                                          gws.nbytes if wsb is None else wsb, None)

    for flags in (Cz | L.SMOOTH_T | L.SMOOTH_H, Cz | L.SMOOTH_T | L.SMOOTH_W, Cz, Cz | L.SMOOTH_H | L.SMOOTH_W):
        assert call(flags) == L.EINVAL
        assert b"KCCOT_SMOOTH_CAUSAL_T" in L.lib.kccot_last_error()
        assert L.lib.kccot_smooth_bwd_f32(gin.ptr, gin.ptr, gmx.ptr, *shape, 1.3, 3, flags, gout.ptr, gws.ptr, gws.nbytes,
                                          None) == L.EINVAL
        assert b"KCCOT_SMOOTH_CAUSAL_T" in L.lib.kccot_last_error()
    assert call(Cz | L.SMOOTH_T, wsb=gws.nbytes - 1) == L.EWORKSPACE
    assert L.lib.kccot_smooth_bwd_f32(gin.ptr, gin.ptr, gmx.ptr, *shape, 1.3, 3, Cz | L.SMOOTH_T, gout.ptr, gws.ptr,
                                      gws.nbytes - 1, None) == L.EWORKSPACE
    assert call(Cz | L.SMOOTH_T, radius=8) == L.EUNSUPPORTED
    _verify(gin, gout, gmx, gws)
    assert all(torch.equal(b.payload(), p) for b, p in zip((gout, gmx, gws), before))


def test_python_method_matches_the_oracle_and_its_gradient():
    from kccotgan_amd.data_utils import KernelSmoothing
    shape = (2, 4, 9, 8, 1)
    gen = torch.Generator().manual_seed(31)
    x, g = torch.rand(shape, generator=gen), torch.randn(shape, generator=gen)
    ks = KernelSmoothing()                      # temporal radius 3
    xc = x.cuda().requires_grad_(True)
    out = ks.causal_temporal_convolution(xc, 1.3)
    (out * g.cuda()).sum().backward()
    ref, din_ref = oracle_grad(x, g, 1.3, ks.temporal_radius)
    assert float((out.detach().cpu().double() - ref).abs().max()) <= ATOL_FWD and float(out.max()) == 1.0
    assert float((xc.grad.cpu().double() - din_ref).abs().max()) <= DIN_TOL * float(din_ref.abs().max())
    sym = ks.temporal_convolution(x.cuda(), 1.3)
    assert not torch.allclose(sym, out.detach(), atol=1e-3)


def test_trainer_runs_one_iteration_with_the_causal_kernel(monkeypatch):
    """KCCOTTrainer(kernel="1d_causal") at the smallest configuration of tests/test_gpu_train_step.py (and in its conservative
    convolution mode)."""
    from kccotgan_amd import gan
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2
    tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="1d_causal",
                      warmup=10, device="cuda:0")
    x = torch.rand(B, H, T, W, C, device="cuda:0")
    calls = []
    real = tr.gaussian_kernel.causal_temporal_convolution
    monkeypatch.setattr(tr.gaussian_kernel, "causal_temporal_convolution", lambda v, s: (calls.append(1), real(v, s))[1])
    pm, loss = tr.train_iteration(x)
    assert calls and torch.isfinite(pm) and torch.isfinite(loss)
