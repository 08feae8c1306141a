"""The anisotropic 3-D kernel smoothing (include/kccot_smooth_aniso.h) on the GPU against the fp64 oracle of
tests/smooth_aniso_oracle.py, run on the device.

Tolerances (the project's own, tests/test_gpu_smoothing_fp64.py and tests/test_gpu_smooth_sigma.py):
  forward   |out - ref| <= 4e-6, max(out) == 1.0 exactly, the arg-max sets agree (inputs tie-free: the fp64 gap between the
            maximum and the runner-up of ref exceeds 1e-5 -- `video` builds such inputs, checked on the CPU for the seeds used);
  backward  |din - ref| <= 1e-5 max|ref|, the oracle's u taken from the kernel's own out and m;
  dsigma    each component within 1e-5 Y of its fp64 value, Y_t = sum |u| (|A_h| |A_w| |A'_t| |x|), Y_s analogously; a radius-0
            group and underflowing taps give exactly 0.  The grid test prints the largest measured ratio."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import abi_guard as ag
import smooth_aniso_oracle as ao
import smooth_sigma_oracle as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
FWD_TOL, BWD_TOL, DS_BOUND, GAP = 4e-6, 1e-5, 1e-5, 1e-5
SHAPES = [(2, 8, 9, 8, 1), (3, 7, 11, 13, 2), (1, 16, 8, 64, 1), (1, 5, 4, 6, 5), (2, 64, 30, 64, 1)]
RADII = [(1, 3), (3, 1), (2, 4), (7, 3), (3, 7), (0, 3), (3, 0), (0, 0)]
SIGMAS = [(0.7, 5.0), (5.0, 0.7), (1.3, 1.3), (0.03, 2.0), (2.0, 0.03)]


def allowed(shape, rt, rs, causal):
    """REFLECT needs radius < the length of every symmetric axis; a causal T takes any radius"""
    B, H, T, W, C = shape
    return (causal or rt < T) and rs < H and rs < W


def rand(shape, seed, normal=False, device=DEV):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=gen) if normal else torch.rand(shape, generator=gen)
    if device != "cpu":
        _lib()          # (kccotgan_amd before the first CUDA call: kccotgan_amd/__init__.py)
    return t.to(device)


def video(shape, seed, device=DEV):
    """A tie-free input by construction: uniform noise of amplitude 0.1 under one bump of height 1 and width 1.5 in (H, T, W)
    (sample 0, channel 0).  Every stencil here is symmetric or one-sided and positive, so the bump keeps one strict maximum;
    the tests still assert the fp64 gap of every case (checked on the CPU for the seeds used)."""
    B, H, T, W, C = shape
    x = 0.1 * rand(shape, seed, device="cpu")
    ax = [torch.arange(n, dtype=torch.float32) - n // 2 for n in (H, T, W)]
    d2 = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2
    x[0, :, :, :, 0] += torch.exp(-d2 / (2 * 1.5 ** 2))
    return x.to(device)


def _lib():
    from kccotgan_amd import _lib
    return _lib


def _ws(t):
    nb = _lib().lib.kccot_smooth_aniso_workspace_bytes(*t.shape)
    return torch.empty(nb, dtype=torch.uint8, device=t.device), nb


def k_fwd(x, cfg, flags=0, mx=None):
    L = _lib()
    st, ss, rt, rs, causal = cfg
    out = torch.full_like(x, float("nan"))
    mx = torch.full((1,), float("nan"), device=x.device) if mx is None else mx
    ws, nb = _ws(x)
    rc = L.lib.kccot_smooth_aniso_fwd_f32(x.data_ptr(), *x.shape, st, rt, ss, rs, flags | (ao.CAUSAL_T if causal else 0),
                                          out.data_ptr(), mx.data_ptr(), ws.data_ptr(), nb, L.stream_of(x))
    assert rc == 0, L.lib.kccot_last_error()
    torch.cuda.synchronize()
    return out, mx


def k_bwd(g, out, mx, cfg, stats=None, flags=0):
    """stats None: the one-call backward; else the sharded entry with `flags` (STATS_ONLY returns None)"""
    L = _lib()
    st, ss, rt, rs, causal = cfg
    din = torch.full_like(out, float("nan"))
    ws, nb = _ws(out)
    fl = flags | (ao.CAUSAL_T if causal else 0)
    if stats is None:
        rc = L.lib.kccot_smooth_aniso_bwd_f32(g.data_ptr(), out.data_ptr(), mx.data_ptr(), *out.shape, st, rt, ss, rs, fl,
                                              din.data_ptr(), ws.data_ptr(), nb, L.stream_of(out))
    else:
        rc = L.lib.kccot_smooth_aniso_bwd_sharded_f32(g.data_ptr(), out.data_ptr(), mx.data_ptr(), stats.data_ptr(), *out.shape,
                                                      st, rt, ss, rs, fl, None if flags & ao.STATS_ONLY else din.data_ptr(),
                                                      ws.data_ptr(), nb, L.stream_of(out))
    assert rc == 0, L.lib.kccot_last_error()
    torch.cuda.synchronize()
    return None if flags & ao.STATS_ONLY else din


def k_dsigma(x, g, out, mx, cfg, stats=None):
    L = _lib()
    st, ss, rt, rs, causal = cfg
    res = torch.full((2,), float("nan"), device=x.device)
    ws, nb = _ws(x)
    rc = L.lib.kccot_smooth_aniso_dsigma_f32(x.data_ptr(), g.data_ptr(), out.data_ptr(), mx.data_ptr(),
                                             None if stats is None else stats.data_ptr(), *x.shape, st, rt, ss, rs,
                                             ao.CAUSAL_T if causal else 0, res.data_ptr(), ws.data_ptr(), nb, L.stream_of(x))
    assert rc == 0, L.lib.kccot_last_error()
    torch.cuda.synchronize()
    return res


def check_forward(x, out, mx, cfg, tie_free=True):
    st, ss, rt, rs, causal = cfg
    ref, m, s = ao.forward(x, so.f32(st), so.f32(ss), rt, rs, causal)
    if tie_free:
        top = torch.topk(ref.flatten(), 2).values
        assert float(top[0] - top[1]) > GAP, ("the input is not tie-free", cfg, float(top[0] - top[1]))
        assert torch.equal(out == 1.0, ref == 1.0), "arg-max sets differ"
    err = float((out.double() - ref).abs().max())
    assert float(out.max()) == 1.0 and err <= FWD_TOL, (cfg, err, float(out.max()))
    assert abs(float(mx) - float(m)) <= FWD_TOL * float(m)
    return err


def check_backward(g, out, mx, din, cfg, stats=None):
    st, ss, rt, rs, causal = cfg
    ref = ao.adjoint(so.upstream(g, out, mx, stats), so.f32(st), so.f32(ss), rt, rs, causal)
    scale = float(ref.abs().max())
    err = float((din.double() - ref).abs().max())
    assert err <= BWD_TOL * scale, (cfg, err, scale)
    return err / scale if scale > 0 else 0.0


def check_dsigma(x, g, out, mx, got, cfg, stats=None):
    """got: the two floats (or sums of shard partials).  Returns the two ratios |got - ref| / Y."""
    st, ss, rt, rs, causal = cfg
    (rt_ref, rs_ref), (yt, ys) = ao.dsigma_ref(x, g, out, mx, so.f32(st), so.f32(ss), rt, rs, causal, stats)
    ratios = []
    for name, v, ref, y, r, sig in (("t", float(got[0]), rt_ref, yt, rt, st), ("s", float(got[1]), rs_ref, ys, rs, ss)):
        if r == 0 or so.all_offdiagonal_taps_underflow(sig, r):
            assert v == 0.0, (name, cfg, v)
            ratios.append(0.0)
            continue
        assert abs(v - ref) <= DS_BOUND * y, (name, cfg, v, ref, y)
        ratios.append(abs(v - ref) / y if y > 0 else 0.0)
    return ratios


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grid_forward_backward_and_dsigma_meet_their_bounds(shape, causal):
    x = video(shape, 12)
    g = rand(shape, 13, normal=True)
    radii = RADII + ([(7, 2)] if causal and shape == (1, 5, 4, 6, 5) else [])       # causal: radius_t >= T
    worst, ran = [0.0, 0.0, 0.0, 0.0], 0
    for rt, rs in radii:
        if not allowed(shape, rt, rs, causal):
            continue
        for st, ss in SIGMAS:
            cfg = (st, ss, rt, rs, causal)
            out, mx = k_fwd(x, cfg)
            e_f = check_forward(x, out, mx, cfg)
            din = k_bwd(g, out, mx, cfg)
            e_b = check_backward(g, out, mx, din, cfg)
            r_t, r_s = check_dsigma(x, g, out, mx, k_dsigma(x, g, out, mx, cfg), cfg)
            worst = [max(a, b) for a, b in zip(worst, (e_f, e_b, r_t, r_s))]
            ran += 1
    print("worst %s causal %d over %d cases: fwd %.3e bwd/max %.3e dsigma_t/Y %.3e dsigma_s/Y %.3e" % ((shape, causal, ran) + tuple(worst)))
    assert ran >= (15 if shape == (1, 5, 4, 6, 5) else 25)


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
@pytest.mark.parametrize("shape", [(2, 8, 9, 8, 1), (2, 64, 30, 64, 1)], ids=["small", "cfg"])
@pytest.mark.parametrize("r", [3, 4])
def test_isotropic_limit_agrees_with_the_isotropic_entry_points(r, shape, causal):
    from kccotgan_amd import data_utils as d
    sigma = 1.3
    axes = d.CAUSAL3 if causal else 7
    form = "causalTHW" if causal else "THW"
    x = video(shape, 21)
    g = rand(shape, 22, normal=True)
    cfg = (sigma, sigma, r, r, causal)
    out, mx = k_fwd(x, cfg)
    out_i, mx_i = d._fwd(x, sigma, r, axes)
    assert float((out - out_i).abs().max()) <= FWD_TOL
    din, din_i = k_bwd(g, out, mx, cfg), d._bwd(g, out_i, mx_i, sigma, r, axes)
    assert float((din - din_i).abs().max()) <= BWD_TOL * float(din_i.abs().max())
    got = k_dsigma(x, g, out, mx, cfg)
    iso = float(d._dsigma(x, g, out_i, mx_i, None, sigma, r, axes, torch.zeros(1)))
    _, (yt, ys) = ao.dsigma_ref(x, g, out, mx, so.f32(sigma), so.f32(sigma), r, r, causal)
    _, y_iso = so.dsigma_ref(x, g, out_i, mx_i, so.f32(sigma), r, form)
    print("isotropic r %d causal %d: dt + ds %.9e iso %.9e" % (r, causal, float(got[0]) + float(got[1]), iso))
    assert abs(float(got[0]) + float(got[1]) - iso) <= DS_BOUND * (yt + ys) + DS_BOUND * y_iso


# (1,2,9,300,3) is listed with r = (4,4); REFLECT along H = 2 allows radius_s <= 1, so that case runs at (4,1)
TILED = [((1, 4, 700, 6, 1), (3, 2)), ((1, 5, 6, 5, 600), (2, 2)), ((1, 2, 9, 300, 3), (4, 1)), ((70, 3, 5, 4, 1), (1, 1))]


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
@pytest.mark.parametrize("shape,r", TILED, ids=lambda v: "x".join(map(str, v)))
def test_tiles_cut_along_t_c_and_w(shape, r, causal):
    cfg = (1.3, 2.0, r[0], r[1], causal)
    x = video(shape, 61)
    g = rand(shape, 62, normal=True)
    out, mx = k_fwd(x, cfg)
    check_forward(x, out, mx, cfg)
    check_backward(g, out, mx, k_bwd(g, out, mx, cfg), cfg)
    check_dsigma(x, g, out, mx, k_dsigma(x, g, out, mx, cfg), cfg)


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
@pytest.mark.parametrize("kind", ["copy", "constant"])
def test_tied_maxima_share_the_correction(kind, causal):
    shape, cfg = (2, 8, 9, 8, 1), (1.3, 2.0, 2, 3, causal)
    if kind == "copy":
        half = rand((1,) + shape[1:], 23)
        x = torch.cat([half, half]).contiguous()
    else:
        x = torch.full(shape, 0.7, device=DEV)
    g = rand(shape, 24, normal=True)
    out, mx = k_fwd(x, cfg)
    check_forward(x, out, mx, cfg, tie_free=False)
    ties = int((out == 1.0).sum())
    assert ties == 2 if kind == "copy" else ties >= 2
    check_backward(g, out, mx, k_bwd(g, out, mx, cfg), cfg)
    check_dsigma(x, g, out, mx, k_dsigma(x, g, out, mx, cfg), cfg)


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
@pytest.mark.parametrize("shape", [(2, 8, 9, 8, 1), (2, 64, 30, 64, 1)], ids=["small", "cfg"])
def test_sharded_protocol_is_bit_equal_to_the_one_call_forms(shape, causal):
    cfg = (1.3, 5.0, 2, 3, causal)
    x = video(shape, 31)
    g = rand(shape, 32, normal=True)
    out, mx = k_fwd(x, cfg)
    din = k_bwd(g, out, mx, cfg)
    whole = k_dsigma(x, g, out, mx, cfg)
    shards = [(x[b:b + 1].contiguous(), g[b:b + 1].contiguous()) for b in range(shape[0])]
    # forward: NO_DIVIDE on each, the host max, EXTERNAL_MAX on each
    raws = [k_fwd(xs, cfg, ao.NO_DIVIDE) for xs, _ in shards]
    for (raw, _), (xs, _) in zip(raws, shards):
        s_ref = ao.fields(xs, so.f32(cfg[0]), so.f32(cfg[1]), cfg[2], cfg[3], causal)[0]
        assert float((raw.double() - s_ref).abs().max()) <= FWD_TOL * float(s_ref.max()), "NO_DIVIDE leaves s"
    gmx = torch.stack([m for _, m in raws]).max().reshape(1)
    assert ag.same_bits(gmx, mx)
    outs = [k_fwd(xs, cfg, ao.EXTERNAL_MAX, gmx.clone())[0] for xs, _ in shards]
    assert ag.same_bits(torch.cat(outs), out), "the sharded forward differs from the one-call forward"
    # backward: STATS_ONLY on each, the sum, EXTERNAL_STATS on each
    stats = []
    for (_, gs), o in zip(shards, outs):
        st = torch.full((2,), float("nan"), device=DEV)
        assert k_bwd(gs, o, gmx, cfg, st, ao.STATS_ONLY) is None
        stats.append(st)
    total = torch.stack(stats).sum(0)
    assert float(total[1]) == float((out == 1.0).sum())
    dins = [k_bwd(gs, o, gmx, cfg, total.clone(), ao.EXTERNAL_STATS) for (_, gs), o in zip(shards, outs)]
    assert ag.same_bits(torch.cat(dins), din), "the sharded backward differs from the one-call backward"
    # dsigma: the shards' partials add up; identical calls, identical bits
    parts = [k_dsigma(xs, gs, o, gmx, cfg, total) for (xs, gs), o in zip(shards, outs)]
    check_dsigma(x, g, out, mx, torch.stack(parts).double().sum(0), cfg)
    check_dsigma(x, g, out, mx, whole, cfg)
    assert ag.same_bits(whole, k_dsigma(x, g, out, mx, cfg)) and ag.same_bits(din, k_bwd(g, out, mx, cfg))
    assert ag.same_bits(out, k_fwd(x, cfg)[0])


GUARD_CASES = [((1, 16, 8, 64, 1), (3, 3), 0), ((3, 7, 11, 13, 2), (7, 3), 4), ((1, 5, 4, 6, 5), (2, 2), 12)]


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
@pytest.mark.parametrize("shape,r,offset", GUARD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_nothing_is_written_outside_the_buffers(shape, r, offset, causal):
    """Guard zones around out, din, dsigma_out, max_inout, stats_inout and the workspace (handed in at exactly the queried size,
    pointers with only 4-byte alignment where offset != 0); the results equal those of the plain calls."""
    L = _lib()
    lib = L.lib
    cfg = (1.3, 2.0, r[0], r[1], causal)
    fl = ao.CAUSAL_T if causal else 0
    x = video(shape, 41)
    g = rand(shape, 42, normal=True)
    out, mx = k_fwd(x, cfg)
    din = k_bwd(g, out, mx, cfg)
    ds = k_dsigma(x, g, out, mx, cfg)
    nb = lib.kccot_smooth_aniso_workspace_bytes(*shape)
    nbytes = x.numel() * 4
    gx, gg, go, gm = (ag.guarded_input(n, t, offset) for n, t in (("in", x), ("gout", g), ("out", out), ("max_in", mx)))
    inputs = (gx, gg, go, gm)
    before = [b.payload().clone() for b in inputs]
    tail = (cfg[0], cfg[2], cfg[1], cfg[3])
    stream = L.stream_of(x)

    def done(rc, *bufs):
        torch.cuda.synchronize()
        assert rc == 0, lib.kccot_last_error()
        for b in inputs + bufs:
            assert b.verify() is None, b.verify()
        for b, was in zip(inputs, before):
            assert torch.equal(b.payload(), was), b.name

    new = lambda n, kind, name: ag.guarded(n, kind, name, offset)
    # forward: one call; NO_DIVIDE then EXTERNAL_MAX
    o, m, ws = new(nbytes, "output", "out"), new(4, "output", "max_inout"), new(nb, "workspace", "ws")
    done(lib.kccot_smooth_aniso_fwd_f32(gx.ptr, *shape, *tail, fl, o.ptr, m.ptr, ws.ptr, nb, stream), o, m, ws)
    assert ag.same_bits(o.view(torch.float32, shape), out) and ag.same_bits(m.view(torch.float32, (1,)), mx)
    o, m, ws = new(nbytes, "output", "out"), new(4, "output", "max_inout"), new(nb, "workspace", "ws")
    done(lib.kccot_smooth_aniso_fwd_f32(gx.ptr, *shape, *tail, fl | ao.NO_DIVIDE, o.ptr, m.ptr, ws.ptr, nb, stream), o, m, ws)
    assert ag.same_bits(m.view(torch.float32, (1,)), mx)
    o, ws = new(nbytes, "output", "out"), new(nb, "workspace", "ws")
    done(lib.kccot_smooth_aniso_fwd_f32(gx.ptr, *shape, *tail, fl | ao.EXTERNAL_MAX, o.ptr, m.ptr, ws.ptr, nb, stream), o, m, ws)
    assert ag.same_bits(o.view(torch.float32, shape), out) and ag.same_bits(m.view(torch.float32, (1,)), mx)
    # backward: one call; STATS_ONLY then EXTERNAL_STATS
    d_, ws = new(nbytes, "output", "din"), new(nb, "workspace", "ws")
    done(lib.kccot_smooth_aniso_bwd_f32(gg.ptr, go.ptr, gm.ptr, *shape, *tail, fl, d_.ptr, ws.ptr, nb, stream), d_, ws)
    assert ag.same_bits(d_.view(torch.float32, shape), din)
    s_, d_, ws = new(8, "output", "stats_inout"), new(nbytes, "output", "din"), new(nb, "workspace", "ws")
    done(lib.kccot_smooth_aniso_bwd_sharded_f32(gg.ptr, go.ptr, gm.ptr, s_.ptr, *shape, *tail, fl | ao.STATS_ONLY, d_.ptr, ws.ptr,
                                                nb, stream), s_, d_, ws)
    assert bool(ag.unwritten(d_.view(torch.float32, shape)).all()), "STATS_ONLY touched din"
    ws = new(nb, "workspace", "ws")
    done(lib.kccot_smooth_aniso_bwd_sharded_f32(gg.ptr, go.ptr, gm.ptr, s_.ptr, *shape, *tail, fl | ao.EXTERNAL_STATS, d_.ptr,
                                                ws.ptr, nb, stream), s_, d_, ws)
    assert ag.same_bits(d_.view(torch.float32, shape), din)
    # dsigma: without and with stats_in
    for stats_ptr in (None, s_.ptr):
        r_, ws = new(8, "output", "dsigma_out"), new(nb, "workspace", "ws")
        done(lib.kccot_smooth_aniso_dsigma_f32(gx.ptr, gg.ptr, go.ptr, gm.ptr, stats_ptr, *shape, *tail, fl, r_.ptr, ws.ptr, nb,
                                               stream), s_, r_, ws)
        assert ag.same_bits(r_.view(torch.float32, (2,)), ds)
    # refused: one byte short -- nothing is written
    o, m, ws = new(nbytes, "output", "out"), new(4, "output", "max_inout"), new(nb, "workspace", "ws")
    assert lib.kccot_smooth_aniso_fwd_f32(gx.ptr, *shape, *tail, fl, o.ptr, m.ptr, ws.ptr, nb - 1, stream) == L.EWORKSPACE
    torch.cuda.synchronize()
    assert bool(ag.unwritten(o.view(torch.float32, shape)).all()) and bool(ag.unwritten(m.view(torch.float32, (1,))).all())
    assert bool((ws.payload().view(torch.int32) == ag._s32(ag.GUARD_WORD)).all())


class _Counter:
    """counts the calls of the anisotropic backward and dsigma entry points that go through _lib.lib"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {"bwd": 0, "dsigma": 0}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        key = {"kccot_smooth_aniso_bwd_f32": "bwd", "kccot_smooth_aniso_dsigma_f32": "dsigma"}.get(name)
        if key is None:
            return fn

        def counted(*a):
            self.calls[key] += 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("causal", [False, True], ids=["sym", "causal"])
def test_public_api_returns_the_entry_points_values(causal, monkeypatch):
    from kccotgan_amd import _lib as L, data_utils as d
    ks = d.KernelSmoothing(4, 6)                     # radius_t = 2, radius_s = 3
    shape = (2, 8, 9, 8, 2)
    st, ss = 1.3, 2.5
    cfg = (st, ss, 2, 3, causal)
    x0 = video(shape, 51)
    w = rand(shape, 52, normal=True)
    counter = _Counter(L.lib)
    monkeypatch.setattr(d, "lib", counter)
    out, mx = k_fwd(x0, cfg)
    din = k_bwd(w, out, mx, cfg)
    ds = k_dsigma(x0, w, out, mx, cfg)

    # float sigmas: din only
    xa = x0.clone().requires_grad_(True)
    outa = ks.anisotropic_gaussian_convolution3D(xa, st, ss, causal=causal)
    (outa * w).sum().backward()
    assert counter.calls == {"bwd": 1, "dsigma": 0}
    assert ag.same_bits(outa.detach(), out) and ag.same_bits(xa.grad, din)
    # both learnable: the same out and din, both gradients in the sigma's shape, dtype and device
    xb = x0.clone().requires_grad_(True)
    sig_t = torch.tensor(st, device=DEV, requires_grad=True)
    sig_s = torch.tensor([ss], dtype=torch.float64, requires_grad=True)
    outb = ks.anisotropic_gaussian_convolution3D(xb, sig_t, sig_s, causal=causal)
    (outb * w).sum().backward()
    assert counter.calls == {"bwd": 2, "dsigma": 1}
    assert ag.same_bits(outb.detach(), out) and ag.same_bits(xb.grad, din)
    assert sig_t.grad.shape == () and sig_t.grad.dtype == torch.float32 and sig_t.grad.device == sig_t.device
    assert sig_s.grad.shape == (1,) and sig_s.grad.dtype == torch.float64 and sig_s.grad.device.type == "cpu"
    assert ag.same_bits(sig_t.grad.reshape(1), ds[0:1]) and float(sig_s.grad) == float(ds[1])
    # one learnable sigma and no gradient for the input: no din, one dsigma call, the other component is dropped
    sig_s2 = torch.tensor(ss, device=DEV, requires_grad=True)
    (ks.anisotropic_gaussian_convolution3D(x0, torch.tensor(st), sig_s2, causal=causal) * w).sum().backward()
    assert counter.calls == {"bwd": 2, "dsigma": 2} and ag.same_bits(sig_s2.grad.reshape(1), ds[1:2])
    sig_t2 = torch.tensor(st, device=DEV, requires_grad=True)
    xc = x0.clone().requires_grad_(True)
    (ks.anisotropic_gaussian_convolution3D(xc, sig_t2, ss, causal=causal) * w).sum().backward()
    assert counter.calls == {"bwd": 3, "dsigma": 3}
    assert ag.same_bits(sig_t2.grad.reshape(1), ds[0:1]) and ag.same_bits(xc.grad, din)


def test_world_size_one_sharded_equals_unsharded(tmp_path):
    """One child process: gloo over a file store, world size 1 -- KernelSmoothing(sharded=True) equals the unsharded call bit
    for bit in out, x.grad and both sigma gradients, for both T forms."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "smooth_aniso_world1.py"), str(tmp_path / "store")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "world1 ok 2" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("kernel", ["3d_aniso", "3d_aniso_causal"])
def test_trainer_runs_one_iteration_with_a_sigma_pair(kernel, monkeypatch):
    from kccotgan_amd import gan
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2          # the smallest configuration of tests/test_gpu_train_step.py
    tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel=kernel, warmup=10,
                      device=DEV, temporal_kernel_size=4)
    assert (tr.gaussian_kernel.temporal_radius, tr.gaussian_kernel.spatial_radius) == (2, 3)
    x = torch.rand(B, H, T, W, C, device=DEV)
    snap = lambda ps: [p.detach().clone() for p in ps]
    g0, d0 = snap(tr.g_params), snap(tr.d_params)
    pm, loss = tr.train_iteration(x, sigma=(1.0, 3.0))
    changed = lambda a, b: any(not torch.equal(p, q) for p, q in zip(a, b))
    assert torch.isfinite(pm) and torch.isfinite(loss)
    assert changed(g0, snap(tr.g_params)) and changed(d0, snap(tr.d_params))
    with pytest.raises(ValueError, match=kernel):
        tr.train_iteration(x, sigma=5.0)
