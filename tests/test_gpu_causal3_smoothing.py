"""The causal 3-D smoothing (include/kccot_smooth_causal3.h; NOT reference behaviour: that header is the specification) on
guarded buffers (tests/abi_guard.py) against a float64 oracle written out below, term by term from the definition:

    a[t] = sum_{d=0}^{min(r,t)} w_d x[t-d] / Z_t,  w_d = exp(-d^2 / (2 sigma^2)),  Z_t = sum_{d=0}^{min(r,t)} w_d      (T, causal)
    s    = H(W(a)),  the normalised (2r+1)-tap Gaussian with REFLECT borders along W, then along H               (symmetric)
    out  = s / max(s)

Tolerances are the ones tests/test_gpu_smoothing_fp64.py holds the symmetric 3-D call to: forward 4e-6 absolute, din 1e-5 of
max|din_ref|, max(out) == 1.0 exactly.  The gradient reference is fp64 autograd through the oracle; torch's amax splits the
gradient evenly over tied maxima, which is the library's convention.  Before any GPU call on an input, an fp32 torch
restatement of the definition in the same stage order is held to the same tolerances on the CPU, and the fp64 maximum must
stand more than 1e-5 above the runner-up (the tie test aside): the inputs are fair.

Shapes (B,H,T,W,C), the smallest that reach each path: (2,8,9,8,1) walk-eligible at r = 3 (r = 4 needs T >= 10 and walks at T = 30), float4,
also from pointers offset by 4 bytes (chain, single floats); (1,8,9,8,3) three channels; (2,17,9,16,1) more than one H segment and column tile
(neighbour halos); (1,5,5,5,3) W*C = 15, scalar pieces, chain only; (1,4,2,4,1) r >= T; (1,4,1,4,1) T = 1; (1,8,30,8,1) the
trainer's T.  Every case runs with smooth_fused3 = 2 (the walk wherever eligible) and 0 (chain), smooth_bwd_fold 0 and 2."""
import pytest
import torch

import abi_guard as ag

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SHAPES = [(2, 8, 9, 8, 1), (1, 8, 9, 8, 3), (2, 17, 9, 16, 1), (1, 5, 5, 5, 3), (1, 4, 2, 4, 1), (1, 4, 1, 4, 1), (1, 8, 30, 8, 1)]
SIGMAS = (5.0, 1.3, 0.03)
RADII = (3, 4, 2, 0)
ATOL_FWD, DIN_TOL, MARGIN = 4e-6, 1e-5, 1e-5
PATHS = [(2, 0), (2, 2), (0, 0), (0, 2)]        # (smooth_fused3, smooth_bwd_fold)
PATH_IDS = ["walk_fold0", "walk_fold2", "chain_fold0", "chain_fold2"]


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


def _reflect_conv(x, axis, w, r):
    n = x.shape[axis]
    idx = torch.arange(-r, n + r).abs()
    idx = torch.where(idx >= n, 2 * (n - 1) - idx, idx)
    xp = x.index_select(axis, idx)
    s = torch.zeros_like(x)
    for k in range(2 * r + 1):
        s = s + w[k] * xp.narrow(axis, k, n)
    return s


def smooth(x, sigma, r, dtype=F64, normalise=True):
    """The definition, term by term, on the CPU.  dtype = float64: the oracle.  dtype = float32: the restatement in the
    library's number format and stage order (T, W, H; taps ascending; the reciprocal of Z_t multiplied in after the T sum)."""
    x = x.to(dtype)
    T = x.shape[2]
    coef = torch.tensor(-0.5 / (float(sigma) * float(sigma)), dtype=dtype)
    w = torch.exp(coef * torch.arange(r + 1, dtype=dtype) ** 2)
    s = torch.zeros_like(x)
    for d in range(min(r, T - 1) + 1):
        s[:, :, d:] = s[:, :, d:] + w[d] * x[:, :, :T - d]
    Z = torch.cumsum(w, 0)[torch.arange(T).clamp(max=r)].view(1, 1, T, 1, 1)
    s = s * (1.0 / Z) if dtype == F32 else s / Z
    k = torch.exp(coef * torch.arange(-r, r + 1, dtype=dtype) ** 2)
    k = k / k.sum()
    s = _reflect_conv(_reflect_conv(s, 3, k, r), 1, k, r)
    return s / s.amax() if normalise else s


def _grad(x, g, sigma, r, dtype):
    xd = x.detach().to(dtype).clone().requires_grad_(True)
    out = smooth(xd, sigma, r, dtype)
    (out * g.to(dtype)).sum().backward()
    return out.detach(), xd.grad


_REFS = {}


def reference(key, x, g, sigma, r, ties=False):
    """fp64 output and gradient, computed once per input and shared; the fairness checks run with it (on the CPU)."""
    key = (key, sigma, r)
    if key not in _REFS:
        ref, din_ref = _grad(x, g, sigma, r, F64)
        if not ties:
            top = torch.topk(ref.flatten(), 2).values
            assert float(top[0] - top[1]) > MARGIN, "unfair input %r: runner-up %.3e below the maximum" % (key, float(top[0] - top[1]))
            o32, d32 = _grad(x, g, sigma, r, F32)
            e_f = float((o32.double() - ref).abs().max())
            e_d = float((d32.double() - din_ref).abs().max()) / float(din_ref.abs().max())
            assert e_f <= ATOL_FWD and e_d <= DIN_TOL, "unfair input %r: the fp32 restatement is off by %.2e / %.2e" % (key, e_f, e_d)
        _REFS[key] = (ref, din_ref)
    return _REFS[key]


def _verify(*bufs):
    torch.cuda.synchronize()
    bad = [m for m in (b.verify() for b in bufs) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)


def fwd(L, x, sigma, r, flags=0, mx=None, offset=0, entry="kccot_smooth_causal3_fwd_f32"):
    """The forward entry point on guarded buffers; returns (out, max) on the CPU."""
    shape = tuple(x.shape)
    gin = ag.guarded_input("in", x.cuda(), offset)
    gout = ag.guarded(x.numel() * 4, "output", "out", offset)
    gmx = ag.guarded(4, "output", "max_inout")
    if mx is not None:
        gmx.view(F32, (1,)).copy_(mx)
    gws = ag.guarded(int(L.lib.kccot_smooth_workspace_bytes(*shape)), "workspace", "ws")
    rc = getattr(L.lib, entry)(gin.ptr, *shape, sigma, r, flags, gout.ptr, gmx.ptr, gws.ptr, gws.nbytes, None)
    assert rc == 0, L.lib.kccot_last_error()
    _verify(gin, gout, gmx, gws)
    assert torch.equal(gin.view(F32, shape).cpu(), x.cpu()), "the input was written"
    return gout.view(F32, shape).cpu(), gmx.view(F32, (1,)).cpu()


def bwd(L, g, out, mx, sigma, r, stats=None, offset=0):
    """kccot_smooth_causal3_bwd_f32, or the sharded entry point: stats == "only" returns the two sums, a tensor is handed in."""
    shape = tuple(out.shape)
    gg, go = ag.guarded_input("gout", g.cuda(), offset), ag.guarded_input("out", out.cuda(), offset)
    gmx = ag.guarded_input("max_in", mx.cuda())
    gdin = ag.guarded(out.numel() * 4, "output", "din", offset)
    gws = ag.guarded(int(L.lib.kccot_smooth_workspace_bytes(*shape)), "workspace", "ws")
    if stats is None:
        rc = L.lib.kccot_smooth_causal3_bwd_f32(gg.ptr, go.ptr, gmx.ptr, *shape, sigma, r, 0, gdin.ptr, gws.ptr, gws.nbytes, None)
        gst = gmx
    else:
        only = isinstance(stats, str)
        gst = ag.guarded(8, "output", "stats_inout") if only else ag.guarded_input("stats_inout", stats.cuda())
        rc = L.lib.kccot_smooth_causal3_bwd_sharded_f32(gg.ptr, go.ptr, gmx.ptr, gst.ptr, *shape, sigma, r,
                                                        L.SMOOTH_STATS_ONLY if only else L.SMOOTH_EXTERNAL_STATS, gdin.ptr,
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
        y[0, shape[1] // 2, 1, 2, 0] = 3.0
        yield "early", y


@pytest.mark.parametrize("f3,fold", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward_against_fp64(L, shape, f3, fold):
    """Every sigma and every radius the REFLECT rule allows (3 and 4 compiled in, 2 and 0 through the generic stages), forward and
    adjoint; the float4 shape also from pointers that are only 4-byte aligned.  Canaries behind out, din, max_inout and the
    workspace are checked in every call."""
    g = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    fails = []
    for kind, x in _inputs(shape, sum(shape)):
        for sigma in SIGMAS:
            for r in RADII:
                if r >= min(shape[1], shape[3]):
                    continue
                ref, din_ref = reference((shape, kind), x, g, sigma, r)
                for offset in ((0, 4) if shape == SHAPES[0] else (0,)):
                    with L.options(smooth_fused3=f3, smooth_bwd_fold=fold):
                        out, mx = fwd(L, x, sigma, r, offset=offset)
                        din = bwd(L, g, out, mx, sigma, r, offset=offset)
                    e_fwd = float((out.double() - ref).abs().max())
                    e_din = float((din.double() - din_ref).abs().max()) / float(din_ref.abs().max())
                    tag = "%s %-6s sigma=%-4g r=%d offset=%d fused3=%d fold=%d" % (shape, kind, sigma, r, offset, f3, fold)
                    print("%s: fwd %.2e  din %.2e  max(out) %r" % (tag, e_fwd, e_din, float(out.max())))
                    if float(out.max()) != 1.0:
                        fails.append("%s: max(out) = %r" % (tag, float(out.max())))
                    if not e_fwd <= ATOL_FWD:
                        fails.append("%s: forward %.3e > %.0e" % (tag, e_fwd, ATOL_FWD))
                    if not e_din <= DIN_TOL:
                        fails.append("%s: adjoint %.3e > %.0e" % (tag, e_din, DIN_TOL))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("f3", [2, 0], ids=["walk", "chain"])
@pytest.mark.parametrize("shape,r", [((2, 8, 9, 8, 1), 3), ((2, 17, 9, 16, 1), 3), ((1, 8, 9, 8, 3), 3), ((1, 8, 30, 8, 1), 4)],
                         ids=["float4_r3", "tiles_r3", "c3_r3", "t30_r4"])
def test_frames_up_to_t0_do_not_depend_on_later_frames(L, shape, r, f3):
    """Causality itself: two videos that agree on frames <= t0 and differ after give bit-identical raw sums in frames <= t0, and
    bit-identical normalised frames <= t0 when both runs divide by the same EXTERNAL_MAX.  The symmetric 3-D call on the same
    pair does not, so the comparison can see a leak."""
    t0 = 4
    gen = torch.Generator().manual_seed(11)
    a = torch.rand(shape, generator=gen)
    b = a.clone()
    b[:, :, t0 + 1:] = torch.rand(b[:, :, t0 + 1:].shape, generator=gen)
    with L.options(smooth_fused3=f3):
        ca, ma = fwd(L, a, 1.3, r, L.SMOOTH_NO_DIVIDE)
        cb, mb = fwd(L, b, 1.3, r, L.SMOOTH_NO_DIVIDE)
        assert ag.same_bits(ca[:, :, :t0 + 1], cb[:, :, :t0 + 1])
        assert not torch.equal(ca[:, :, t0 + 1:], cb[:, :, t0 + 1:])
        assert float(ma) == float(ca.max()) and float(mb) == float(cb.max())
        mx = torch.maximum(ma, mb)
        na, _ = fwd(L, a, 1.3, r, L.SMOOTH_EXTERNAL_MAX, mx=mx)
        nb, _ = fwd(L, b, 1.3, r, L.SMOOTH_EXTERNAL_MAX, mx=mx)
        assert ag.same_bits(na[:, :, :t0 + 1], nb[:, :, :t0 + 1])
        assert float(na.max()) <= 1.0 and float(nb.max()) <= 1.0 and max(float(na.max()), float(nb.max())) == 1.0
        axes = L.SMOOTH_T | L.SMOOTH_H | L.SMOOTH_W | L.SMOOTH_NO_DIVIDE
        sa, _ = fwd(L, a, 1.3, r, axes, entry="kccot_smooth_fwd_f32")
        sb, _ = fwd(L, b, 1.3, r, axes, entry="kccot_smooth_fwd_f32")
    assert not torch.equal(sa[:, :, :t0 + 1], sb[:, :, :t0 + 1]), "the symmetric stencil should leak frames > t0"


@pytest.mark.parametrize("shape,r", [((2, 17, 9, 16, 1), 3), ((1, 8, 9, 8, 3), 3), ((1, 8, 30, 8, 1), 4)], ids=["tiles_r3", "c3_r3", "t30_r4"])
def test_walk_and_chain_give_the_same_bits_forward(L, shape, r):
    """The fused walk sums every output in the chain's order (T ascending d then 1 / Z_t, W, H): raw sums, maximum and normalised
    output are bit-identical between the two tiers."""
    x = torch.rand(shape, generator=torch.Generator().manual_seed(17))
    for flags in (L.SMOOTH_NO_DIVIDE, 0):
        with L.options(smooth_fused3=2):
            ow, mw = fwd(L, x, 1.3, r, flags)
        with L.options(smooth_fused3=0):
            oc, mc = fwd(L, x, 1.3, r, flags)
        assert ag.same_bits(ow, oc) and ag.same_bits(mw, mc)


@pytest.mark.parametrize("f3", [2, 0], ids=["walk", "chain"])
def test_space_is_symmetric(L, f3):
    """Flipping the input along H, or along W, flips the raw sums.  Within the forward tolerance, not bit for bit: the taps are
    summed in ascending index, so the flipped input is summed in the opposite order and rounds differently."""
    shape = (2, 17, 9, 16, 1)
    x = torch.rand(shape, generator=torch.Generator().manual_seed(13))
    with L.options(smooth_fused3=f3):
        s, _ = fwd(L, x, 1.3, 3, L.SMOOTH_NO_DIVIDE)
        for axis in (1, 3):
            sf, _ = fwd(L, x.flip(axis).contiguous(), 1.3, 3, L.SMOOTH_NO_DIVIDE)
            err = float((sf.flip(axis) - s).abs().max())
            print("flip along axis %d, fused3=%d: %.2e" % (axis, f3, err))
            assert err <= ATOL_FWD
        # ... and time is not: the flipped video is not the flipped result
        sf, _ = fwd(L, x.flip(2).contiguous(), 1.3, 3, L.SMOOTH_NO_DIVIDE)
        assert float((sf.flip(2) - s).abs().max()) > 1e-2


@pytest.mark.parametrize("f3", [2, 0], ids=["walk", "chain"])
def test_constant_gives_ones_and_frame_zero_is_its_spatial_smoothing(L, f3):
    shape = (2, 8, 9, 8, 1)
    with L.options(smooth_fused3=f3):
        for r in (3, 2):
            ones, _ = fwd(L, torch.full(shape, 0.37), 1.3, r)
            assert float((ones - 1.0).abs().max()) <= ATOL_FWD and float(ones.max()) == 1.0
            x = torch.rand(shape, generator=torch.Generator().manual_seed(5))
            raw, mx = fwd(L, x, 1.3, r, L.SMOOTH_NO_DIVIDE)
            assert float(mx) == float(raw.max())
            hw, _ = fwd(L, x, 1.3, r, L.SMOOTH_H | L.SMOOTH_W | L.SMOOTH_NO_DIVIDE, entry="kccot_smooth_fwd_f32")
            assert float((raw[:, :, 0] - hw[:, :, 0]).abs().max()) <= ATOL_FWD     # a[0] = x[0]: no time smoothing in frame 0
            assert float((raw[:, :, 1:] - hw[:, :, 1:]).abs().max()) > 1e-3


def _tied(n_ties):
    """n_ties identical voxels on a zero background whose stencils do not meet (7 > 2r apart along H or W, or 4 > r along T, so
    no point between two of them collects from both), none within r of a border (no REFLECTed tap reaches one twice), all in frames t >= r,
    where Z_t is the same: their smoothed values are the same fp32 (and fp64) number, and it is the maximum.  Eight share a
    sample, so a workgroup's record overflows (TIE_PER_WG = 4)."""
    shape = (5, 16, 9, 16, 1)
    slots = [(b, h, t, w) for b in range(5) for t in (4, 8) for h in (4, 11) for w in (4, 11)]
    x = torch.zeros(shape)
    for b, h, t, w in slots[:n_ties]:
        x[b, h, t, w, 0] = 1.0
    assert int(x.sum()) == n_ties
    return x


@pytest.mark.parametrize("f3,fold", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("n_ties", [2, 40])
def test_tied_maxima_share_the_correction(L, n_ties, f3, fold):
    """Two tied maxima (the sparse fix-up, three axes) and 40 (above its 32 entries: the dense form), two-pass and folded."""
    x = _tied(n_ties)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
    for sigma in (1.3, 5.0):
        ref, din_ref = reference(("tied", n_ties), x, g, sigma, 3, ties=True)
        assert int((ref == 1).sum()) == n_ties
        with L.options(smooth_fused3=f3, smooth_bwd_fold=fold):
            out, mx = fwd(L, x, sigma, 3)
            din = bwd(L, g, out, mx, sigma, 3)
            stats = bwd(L, g, out, mx, sigma, 3, stats="only")
        assert torch.equal(out == 1, ref == 1) and int(stats[1]) == n_ties
        e_fwd = float((out.double() - ref).abs().max())
        e_din = float((din.double() - din_ref).abs().max()) / float(din_ref.abs().max())
        print("ties %d sigma %g fused3 %d fold %d: fwd %.2e din %.2e" % (n_ties, sigma, f3, fold, e_fwd, e_din))
        assert e_fwd <= ATOL_FWD and e_din <= DIN_TOL


@pytest.mark.parametrize("f3", [2, 0], ids=["walk", "chain"])
@pytest.mark.parametrize("shape", [(2, 4, 8, 8, 1), (2, 8, 9, 8, 1)], ids=["one_partial", "walk_eligible"])
def test_sharded_protocol_on_one_gpu_equals_the_whole_batch(L, shape, f3):
    """The batch cut in two: NO_DIVIDE per half, the larger maximum, EXTERNAL_MAX; STATS_ONLY per half, the sums added,
    EXTERNAL_STATS.  The forward equals the one call on the whole batch bit for bit, the adjoint is within the din tolerance.  In
    the first shape a sample is 256 elements, one workgroup of the sums' first stage, so each half hands back ONE fp32 partial
    sum; the second shape is the smallest the fused walks take (their EXTERNAL_STATS form).  The maximum lies in one half: the
    other half's tie count is 0 and its elements still take their share of the correction's sum."""
    sigma, r = 1.3, 3
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(shape, generator=gen)
    g = torch.randn(shape, generator=gen)
    ref, din_ref = reference(("sharded", shape), x, g, sigma, r)
    with L.options(smooth_fused3=f3, smooth_bwd_fold=0):
        one, m1 = fwd(L, x, sigma, r)
        halves = [slice(0, 1), slice(1, 2)]
        maxima = [fwd(L, x[s], sigma, r, L.SMOOTH_NO_DIVIDE)[1] for s in halves]
        mx = torch.maximum(*maxima)
        out = torch.cat([fwd(L, x[s], sigma, r, L.SMOOTH_EXTERNAL_MAX, mx=mx)[0] for s in halves])
        assert ag.same_bits(mx, m1) and ag.same_bits(out, one)
        assert int((out == 1).sum()) == 1
        parts = [bwd(L, g[s], out[s], mx, sigma, r, stats="only") for s in halves]
        stats = (parts[0].double() + parts[1].double()).float()
        assert int(stats[1]) == 1
        din = torch.cat([bwd(L, g[s], out[s], mx, sigma, r, stats=stats) for s in halves])
    e_din = float((din.double() - din_ref).abs().max()) / float(din_ref.abs().max())
    print("sharded %s fused3 %d: din %.2e" % (shape, f3, e_din))
    assert e_din <= DIN_TOL


def test_argument_rules_leave_the_buffers_untouched(L):
    shape = (2, 8, 9, 8, 1)
    x = torch.rand(shape)
    gin, gout = ag.guarded_input("in", x.cuda()), ag.guarded(x.numel() * 4, "output", "out")
    gmx, gws = ag.guarded(4, "output", "max_inout"), ag.guarded(int(L.lib.kccot_smooth_workspace_bytes(*shape)), "workspace", "ws")
    gst = ag.guarded(8, "output", "stats_inout")
    before = [b.payload().clone() for b in (gout, gmx, gws, gst)]
    lib = L.lib

    def f(flags=0, wsb=None, radius=3, shape=shape, sigma=1.3):
        return lib.kccot_smooth_causal3_fwd_f32(gin.ptr, *shape, sigma, radius, flags, gout.ptr, gmx.ptr, gws.ptr,
                                                gws.nbytes if wsb is None else wsb, None)

    def b(flags=0, wsb=None, radius=3, shape=shape, sigma=1.3):
        return lib.kccot_smooth_causal3_bwd_f32(gin.ptr, gin.ptr, gmx.ptr, *shape, sigma, radius, flags, gout.ptr, gws.ptr,
                                                gws.nbytes if wsb is None else wsb, None)

    def s(flags=None, wsb=None, radius=3, shape=shape, sigma=1.3):
        return lib.kccot_smooth_causal3_bwd_sharded_f32(gin.ptr, gin.ptr, gmx.ptr, gst.ptr, *shape, sigma, radius,
                                                        L.SMOOTH_EXTERNAL_STATS if flags is None else flags | L.SMOOTH_EXTERNAL_STATS,
                                                        gout.ptr, gws.ptr, gws.nbytes if wsb is None else wsb, None)

    for call, name in ((f, b"kccot_smooth_causal3_fwd_f32"), (b, b"kccot_smooth_causal3_bwd_f32"),
                       (s, b"kccot_smooth_causal3_bwd_sharded_f32")):
        for bit in (L.SMOOTH_T, L.SMOOTH_H, L.SMOOTH_W, L.SMOOTH_CAUSAL_T, L.SMOOTH_T | L.SMOOTH_H | L.SMOOTH_W):
            assert call(flags=bit) == L.EINVAL
            assert name in lib.kccot_last_error()
        assert call(wsb=gws.nbytes - 1) == L.EWORKSPACE
        assert call(radius=8) == L.EUNSUPPORTED
        assert call(sigma=0.0) == L.EINVAL
        assert call(shape=(6, 3, 8, 9, 1)) == L.EINVAL and call(shape=(6, 8, 9, 3, 1)) == L.EINVAL      # r >= H, r >= W
    assert f(flags=L.SMOOTH_NO_DIVIDE | L.SMOOTH_EXTERNAL_MAX) == L.EINVAL
    assert b(flags=L.SMOOTH_STATS_ONLY) == L.EINVAL
    assert s(flags=L.SMOOTH_STATS_ONLY) == L.EINVAL         # both stats flags
    _verify(gin, gout, gmx, gws, gst)
    assert all(torch.equal(buf.payload(), p) for buf, p in zip((gout, gmx, gws, gst), before))


@pytest.mark.parametrize("f3", [2, 0], ids=["walk", "chain"])
def test_python_method_matches_the_oracle_and_its_gradient(L, f3):
    from kccotgan_amd.data_utils import KernelSmoothing
    shape = (2, 8, 9, 8, 1)
    gen = torch.Generator().manual_seed(31)
    x, g = torch.rand(shape, generator=gen), torch.randn(shape, generator=gen)
    ks = KernelSmoothing()                      # spatial radius 4
    assert ks.spatial_radius == 4 and ks.temporal_radius == 3
    ref, din_ref = reference(("python", shape), x, g, 1.3, ks.spatial_radius)
    xc = x.cuda().requires_grad_(True)
    with L.options(smooth_fused3=f3):
        out = ks.causal_gaussian_convolution3D(xc, 1.3)
        (out * g.cuda()).sum().backward()
        sym = ks.gaussian_convolution3D(x.cuda(), 1.3)
    assert float((out.detach().cpu().double() - ref).abs().max()) <= ATOL_FWD and float(out.max()) == 1.0
    assert float((xc.grad.cpu().double() - din_ref).abs().max()) <= DIN_TOL * float(din_ref.abs().max())
    assert not torch.allclose(sym, out.detach(), atol=1e-3)


def test_trainer_runs_one_iteration_with_the_causal_3d_kernel(monkeypatch):
    """KCCOTTrainer(kernel="3d_causal") at the smallest configuration of tests/test_gpu_train_step.py (and in its conservative
    convolution mode); the new method is what smooths the real and the generated video."""
    from kccotgan_amd import gan
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2
    tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="3d_causal",
                      warmup=10, device="cuda:0")
    x = torch.rand(B, H, T, W, C, device="cuda:0")
    calls = []
    real = tr.gaussian_kernel.causal_gaussian_convolution3D
    monkeypatch.setattr(tr.gaussian_kernel, "causal_gaussian_convolution3D", lambda v, s: (calls.append(1), real(v, s))[1])
    pm, loss = tr.train_iteration(x)
    assert len(calls) >= 2 and torch.isfinite(pm) and torch.isfinite(loss)
