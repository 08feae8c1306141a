"""d loss / d sigma of the kernel smoothing (kccot_smooth_dsigma_f32, include/kccot_smooth_sigma.h) against the fp64 oracle of
tests/smooth_sigma_oracle.py, run on the device from the kernel's own `out` and maximum.

The bound: |dsigma - dsigma_ref| <= 1e-5 * Y with the yardstick Y = sum |u| * (|A'| |x|) (the same operator with |w'|, w and
|x|): about 100 fp32 roundings per term at r <= 7 over three axes, times 2^-24 = 6e-6, rounded up.  The largest measured
ratio |dsigma - dsigma_ref| / Y is printed by the grid test (DESIGN.md section 4.5.3 records it)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import abi_guard as ag
import smooth_sigma_oracle as so

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BOUND = 1e-5
SHAPES = [(2, 8, 9, 8, 1), (3, 7, 11, 13, 2), (1, 16, 8, 64, 1), (1, 30, 8, 64, 1), (2, 64, 30, 64, 1), (1, 64, 30, 64, 3)]
RADII = (0, 1, 3, 4, 7)
SIGMAS = (5.0, 1.3, 0.3, 0.03)
DEV = "cuda:0"


def _axes(form):
    from kccotgan_amd import data_utils as d
    return d.CAUSAL3 if form == "causalTHW" else so.flags(form)


def _allowed(shape, r, form):
    """REFLECT needs r < the length of every symmetric axis; a causal T takes any radius"""
    B, H, T, W, C = shape
    if form in ("T",) and r >= T:
        return False
    if form == "THW" and r >= T:
        return False
    if form in ("HW", "THW", "causalTHW") and (r >= H or r >= W):
        return False
    return True


def _forward(x, sigma, r, form):
    from kccotgan_amd import data_utils as d
    return d._fwd(x, float(sigma), r, _axes(form))


def _dsigma(x, g, out, mx, sigma, r, form, stats=None):
    from kccotgan_amd import _lib
    B, H, T, W, C = x.shape
    res = torch.full((1,), float("nan"), dtype=torch.float32, device=x.device)
    nb = _lib.lib.kccot_smooth_dsigma_workspace_bytes(B, H, T, W, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    rc = _lib.lib.kccot_smooth_dsigma_f32(x.data_ptr(), g.data_ptr(), out.data_ptr(), mx.data_ptr(),
                                          stats.data_ptr() if stats is not None else None, B, H, T, W, C, float(sigma), r,
                                          so.flags(form), res.data_ptr(), ws.data_ptr(), nb, _lib.stream_of(x))
    assert rc == 0, _lib.lib.kccot_last_error()
    torch.cuda.synchronize()
    return res


def _stats(g, out, mx, sigma, r, form):
    """{sum g*out, n_ties} by the library's stats-only pass"""
    from kccotgan_amd import _lib, data_utils as d
    B, H, T, W, C = out.shape
    stats = torch.zeros(2, dtype=torch.float32, device=out.device)
    nb = _lib.lib.kccot_smooth_workspace_bytes(B, H, T, W, C)
    ws = torch.empty(nb, dtype=torch.uint8, device=out.device)
    _, _, bwd, bits = d._entry(_axes(form))
    rc = bwd(g.data_ptr(), out.data_ptr(), mx.data_ptr(), stats.data_ptr(), B, H, T, W, C, float(sigma), r,
             bits | _lib.SMOOTH_STATS_ONLY, None, ws.data_ptr(), nb, _lib.stream_of(out))
    assert rc == 0, _lib.lib.kccot_last_error()
    return stats


def _ref(u, ds, ya):
    return float((u * ds).sum()), float((u.abs() * ya).sum())


def _rand(shape, seed, normal=False):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=gen) if normal else torch.rand(shape, generator=gen)
    return t.to(DEV)


@pytest.mark.parametrize("form", so.FORMS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grid_meets_the_bound_for_random_and_aligned_gout(shape, form):
    x = _rand(shape, 11)
    g_rand = _rand(shape, 12, normal=True)
    worst, ran = 0.0, 0
    for r in RADII:
        if not _allowed(shape, r, form):
            continue
        for sigma in SIGMAS:
            out, mx = _forward(x, sigma, r, form)
            if r == 0:
                assert float(_dsigma(x, g_rand, out, mx, sigma, r, form)) == 0.0
                ran += 1
                continue
            s32 = so.f32(sigma)
            _, ds = so.fields(x, s32, r, form, False, True)
            _, ya = so.fields(x, s32, r, form, True, True)
            cases = [("random", g_rand)]
            if so.all_offdiagonal_taps_underflow(sigma, r):
                # every e_d, d != 0, underflows: the derivative taps are zero and so is the result, exactly
                assert float(_dsigma(x, g_rand, out, mx, sigma, r, form)) == 0.0
            else:
                cases.append(("aligned", ds.to(torch.float32)))
            for kind, g in cases:
                got = float(_dsigma(x, g, out, mx, sigma, r, form))
                ref, y = _ref(so.upstream(g, out, mx), ds, ya)
                ratio = abs(got - ref) / y if y > 0 else (0.0 if got == ref else float("inf"))
                worst = max(worst, ratio)
                print("%s %s r %d sigma %g %s: got %.9e ref %.9e Y %.4e ratio %.3e" % (shape, form, r, sigma, kind, got, ref, y, ratio))
                if kind == "aligned":
                    assert abs(ref) >= 0.01 * y, (kind, r, sigma, ref, y)      # the bound is <= 1e-3 of the value itself
                assert abs(got - ref) <= BOUND * y, (kind, r, sigma, got, ref, y)
                ran += 1
    print("worst ratio %s %s: %.3e over %d cases" % (shape, form, worst, ran))
    assert ran >= 20


TILED = [((1, 4, 700, 6, 1), 3), ((1, 4, 300, 5, 2), 7), ((1, 5, 6, 5, 600), 2), ((1, 2, 9, 40, 300), 4), ((70, 3, 5, 4, 1), 1),
         ((1, 9, 1, 9, 1), 7), ((2, 3, 2, 3, 5), 2)]


@pytest.mark.parametrize("form", so.FORMS)
@pytest.mark.parametrize("shape,r", TILED, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "r%d" % v)
def test_tiles_cut_along_t_and_c_and_tiny_frames(shape, r, form):
    """Shapes whose plane does not fit one tile: T cut into tiles with REFLECT / causal halo rows (T = 700, 300), channels cut
    (C = 600, and W*C = 12000 merged for the forms without W), many tiny samples, T = 1 and T = 2 (radius >= T for the causal
    forms)."""
    r = max(q for q in (r, 1, 0) if q <= r and _allowed(shape, q, form))
    sigma = 1.3
    x = _rand(shape, 61)
    g = _rand(shape, 62, normal=True)
    out, mx = _forward(x, sigma, r, form)
    got = float(_dsigma(x, g, out, mx, sigma, r, form))
    if r == 0:
        assert got == 0.0
        return
    _, ds = so.fields(x, so.f32(sigma), r, form, False, True)
    _, ya = so.fields(x, so.f32(sigma), r, form, True, True)
    ref, y = _ref(so.upstream(g, out, mx), ds, ya)
    print("tiled %s %s r %d: got %.9e ref %.9e Y %.4e" % (shape, form, r, got, ref, y))      # (T = 1, causal: all three are 0)
    assert abs(got - ref) <= BOUND * y


@pytest.mark.parametrize("form", so.FORMS)
def test_constant_video_and_radius_zero(form):
    shape, r, sigma = (2, 8, 9, 8, 1), 3, 1.3
    x = torch.full(shape, 0.7, device=DEV)
    g = _rand(shape, 5, normal=True)
    out, mx = _forward(x, sigma, r, form)
    got = float(_dsigma(x, g, out, mx, sigma, r, form))
    _, ya = so.fields(x, so.f32(sigma), r, form, True, True)
    y = float((so.upstream(g, out, mx).abs() * ya).sum())
    print("constant %s: dsigma %.3e Y %.3e" % (form, got, y))
    assert abs(got) <= BOUND * y
    xr = _rand(shape, 6)
    out0, mx0 = _forward(xr, sigma, 0, form)
    assert float(_dsigma(xr, g, out0, mx0, sigma, 0, form)) == 0.0


@pytest.mark.parametrize("form", so.FORMS)
def test_tied_maxima_share_the_correction(form):
    shape, r, sigma = (2, 8, 9, 8, 1), 3, 1.3
    half = _rand((1,) + shape[1:], 21)
    x = torch.cat([half, half]).contiguous()
    g = _rand(shape, 22, normal=True)
    out, mx = _forward(x, sigma, r, form)
    assert int((out == 1.0).sum()) >= 2
    got = float(_dsigma(x, g, out, mx, sigma, r, form))
    _, ds = so.fields(x, so.f32(sigma), r, form, False, True)
    _, ya = so.fields(x, so.f32(sigma), r, form, True, True)
    ref, y = _ref(so.upstream(g, out, mx), ds, ya)
    print("ties %s: got %.9e ref %.9e Y %.4e" % (form, got, ref, y))
    assert abs(got - ref) <= BOUND * y


@pytest.mark.parametrize("form", so.FORMS)
@pytest.mark.parametrize("shape", [(2, 8, 9, 8, 1), (2, 64, 30, 64, 1)], ids=["small", "cfg"])
def test_sharded_protocol_stats_and_repeatability(shape, form):
    r, sigma = 3, 1.3
    x = _rand(shape, 31)
    g = _rand(shape, 32, normal=True)
    out, mx = _forward(x, sigma, r, form)
    stats = _stats(g, out, mx, sigma, r, form)
    whole = _dsigma(x, g, out, mx, sigma, r, form)
    again = _dsigma(x, g, out, mx, sigma, r, form)
    given = _dsigma(x, g, out, mx, sigma, r, form, stats)
    assert ag.same_bits(whole, again), "two identical calls differ"
    assert ag.same_bits(whole, given), "stats_in = NULL and the call's own stats handed in differ"
    parts = [float(_dsigma(x[b:b + 1].contiguous(), g[b:b + 1].contiguous(), out[b:b + 1].contiguous(), mx, sigma, r, form, stats))
             for b in range(shape[0])]
    _, ds = so.fields(x, so.f32(sigma), r, form, False, True)
    _, ya = so.fields(x, so.f32(sigma), r, form, True, True)
    ref, y = _ref(so.upstream(g, out, mx), ds, ya)
    print("sharded %s: parts %s whole %.9e ref %.9e Y %.4e" % (form, parts, float(whole), ref, y))
    assert abs(sum(parts) - ref) <= BOUND * y
    assert abs(float(whole) - ref) <= BOUND * y


GUARD_CASES = [((1, 16, 8, 64, 1), 3, 0), ((1, 30, 8, 64, 1), 4, 0), ((3, 7, 11, 13, 2), 3, 4), ((1, 5, 4, 6, 5), 2, 12),
               ((2, 8, 1, 8, 1), 7, 4), ((2, 9, 10, 9, 3), 7, 0)]


@pytest.mark.parametrize("form", so.FORMS)
@pytest.mark.parametrize("shape,r,offset", GUARD_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_nothing_is_written_outside_the_buffers(shape, r, offset, form):
    """Guard zones around the result, the workspace at exactly the queried size and the inputs (pointers with only 4-byte
    alignment where offset != 0); with and without stats_in; a refused call writes nothing at all."""
    from kccotgan_amd import _lib
    r = max(q for q in (r, 3, 1, 0) if q <= r and _allowed(shape, q, form))     # (the form's REFLECT axes may be shorter)
    sigma = 1.3
    B, H, T, W, C = shape
    x = _rand(shape, 41)
    g = _rand(shape, 42, normal=True)
    out, mx = _forward(x, sigma, r, form)
    stats = _stats(g, out, mx, sigma, r, form)
    want = float(_dsigma(x, g, out, mx, sigma, r, form))
    nb = _lib.lib.kccot_smooth_dsigma_workspace_bytes(B, H, T, W, C)
    gx, gg, go = ag.guarded_input("in", x, offset), ag.guarded_input("gout", g, offset), ag.guarded_input("out", out, offset)
    gm, gs = ag.guarded_input("max_in", mx, offset), ag.guarded_input("stats_in", stats, offset)
    inputs = (gx, gg, go, gm, gs)
    before = [b.payload().clone() for b in inputs]

    def call(stats_ptr, res, ws, wsb, radius=r):
        rc = _lib.lib.kccot_smooth_dsigma_f32(gx.ptr, gg.ptr, go.ptr, gm.ptr, stats_ptr, B, H, T, W, C, sigma, radius,
                                              so.flags(form), res.ptr, ws.ptr, wsb, _lib.stream_of(x))
        torch.cuda.synchronize()
        return rc

    for stats_ptr in (None, gs.ptr):
        res, ws = ag.guarded(4, "output", "dsigma_out", offset), ag.guarded(nb, "workspace", "ws", offset)
        assert call(stats_ptr, res, ws, nb) == 0, _lib.lib.kccot_last_error()
        for b in inputs + (res, ws):
            assert b.verify() is None, b.verify()
        for b, was in zip(inputs, before):
            assert torch.equal(b.payload(), was), b.name
        assert float(res.view(torch.float32, (1,))) == want
        # refused: one byte short, and a radius out of range -- result and workspace stay as they were
        for wsb, radius, code in ((nb - 1, r, _lib.EWORKSPACE), (nb, 8, _lib.EINVAL)):
            res, ws = ag.guarded(4, "output", "dsigma_out", offset), ag.guarded(nb, "workspace", "ws", offset)
            assert call(stats_ptr, res, ws, wsb, radius) == code
            assert bool(ag.unwritten(res.view(torch.float32, (1,))).all())
            assert bool((ws.payload().view(torch.int32) == ag._s32(ag.GUARD_WORD)).all())
            assert res.verify() is None and ws.verify() is None


METHODS = ("temporal_convolution", "causal_temporal_convolution", "spatial_convolution", "gaussian_convolution3D",
           "causal_gaussian_convolution3D")


class _Counter:
    """counts the calls of kccot_smooth_dsigma_f32 that go through _lib.lib"""

    def __init__(self, lib):
        self._lib, self.calls, self.last = lib, 0, None

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "kccot_smooth_dsigma_f32":
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


@pytest.mark.parametrize("method,form", list(zip(METHODS, so.FORMS)))
def test_public_api_returns_the_entrys_gradient_and_leaves_the_rest_bit_identical(method, form, monkeypatch):
    from kccotgan_amd import _lib, data_utils as d
    ks = d.KernelSmoothing(6, 6)
    r = 3
    shape = (2, 8, 9, 8, 2)
    x0 = _rand(shape, 51)
    w = _rand(shape, 52, normal=True)
    counter = _Counter(_lib.lib)
    monkeypatch.setattr(d, "lib", counter)

    xa = x0.clone().requires_grad_(True)
    outa = getattr(ks, method)(xa, 1.3)
    (outa * w).sum().backward()
    assert counter.calls == 0

    xb = x0.clone().requires_grad_(True)
    sig = torch.tensor(1.3, device=DEV, requires_grad=True)
    outb = getattr(ks, method)(xb, sig)
    (outb * w).sum().backward()
    assert counter.calls == 1
    assert ag.same_bits(outa.detach(), outb.detach()) and ag.same_bits(xa.grad, xb.grad)
    out, mx = _forward(x0, 1.3, r, form)
    assert ag.same_bits(out, outb.detach())
    direct = _dsigma(x0, w, out, mx, 1.3, r, form)
    assert sig.grad.shape == () and sig.grad.dtype == torch.float32 and sig.grad.device == sig.device
    assert ag.same_bits(sig.grad.reshape(1), direct)

    # a CPU float64 0-dim sigma gets a CPU float64 gradient with the same value
    xc = x0.clone().requires_grad_(True)
    sig64 = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    (getattr(ks, method)(xc, sig64) * w).sum().backward()
    assert sig64.grad.device.type == "cpu" and sig64.grad.dtype == torch.float64 and sig64.grad.shape == ()
    assert float(sig64.grad) == float(direct) and ag.same_bits(xa.grad, xc.grad)
    # only sigma needs a gradient: the same value, no din
    sig2 = torch.tensor([1.3], device=DEV, requires_grad=True)
    (getattr(ks, method)(x0, sig2) * w).sum().backward()
    assert sig2.grad.shape == (1,) and ag.same_bits(sig2.grad, direct)
    # a tensor sigma that does not require a gradient takes the old path: the new entry is not called
    calls = counter.calls
    xd = x0.clone().requires_grad_(True)
    outd = getattr(ks, method)(xd, torch.tensor(1.3, device=DEV))
    (outd * w).sum().backward()
    assert counter.calls == calls and ag.same_bits(outd.detach(), outa.detach()) and ag.same_bits(xd.grad, xa.grad)


def test_world_size_one_sharded_equals_unsharded(tmp_path):
    """One child process: gloo over a file store, world size 1 -- KernelSmoothing(sharded=True) with a tensor sigma equals the
    unsharded call bit for bit in out, x.grad and sigma.grad, for the five methods."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "smooth_sigma_world1.py"), str(tmp_path / "store")],
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "world1 ok 5" in r.stdout, r.stdout[-2000:]
