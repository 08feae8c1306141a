"""Per-frame SSIM, its adjoint and the mean squared error (include/kccot_metrics.h, csrc/ssim.hip) on the GPU against the fp64
oracle of tests/ssim_oracle.py, run on the device, at the shapes of ssim_oracle.GRID.

Tolerances: 4 times the largest error the kernels showed against the fp64 oracle over the grid on an MI355X (the factor covers
the summation-order differences of a later re-tiling), none above the caps of ssim_oracle (which tests/test_ssim_cpu.py shows
a plain float32 evaluation of the definition to stay inside):
    measured  |ssim - ref|            noise 3.253e-07   flat 1.891e-05
              |dy - ref| / max|ref|   noise 4.133e-06
              |mse - ref| / ref       5.173e-08
    allowed   min(4 x measured, cap): 1.30e-06, 5e-05 (the cap: 2.6 x measured), 1.65e-05, 2.07e-07
The grid is the issue's eight shapes and two more at which the kernels cut a row into column and channel tiles.
The grid test prints each figure before it asserts."""
import pytest
import torch

import abi_guard as ag
import ssim_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEASURED = {"ssim_noise": 3.253e-07, "ssim_flat": 1.891e-05, "dy": 4.133e-06, "mse": 5.173e-08}
TOL_SSIM = {"noise": min(4 * MEASURED["ssim_noise"], so.CAP_SSIM["noise"]), "flat": min(4 * MEASURED["ssim_flat"], so.CAP_SSIM["flat"])}
TOL_DY = min(4 * MEASURED["dy"], so.CAP_DY)
TOL_MSE = min(4 * MEASURED["mse"], so.CAP_MSE)
assert TOL_SSIM["noise"] <= so.CAP_SSIM["noise"] and TOL_SSIM["flat"] <= so.CAP_SSIM["flat"]
assert TOL_DY <= so.CAP_DY and TOL_MSE <= so.CAP_MSE
IDS = ["x".join(map(str, c[0])) + "-w%d-%s" % (c[1], c[3]) for c in so.GRID]


def _lib():
    from kccotgan_amd import _lib
    return _lib


def data(kind, shape, seed):
    _lib()              # (kccotgan_amd before the first CUDA call: kccotgan_amd/__init__.py)
    return so.inputs(kind, shape, seed, DEV)


def _done(rc, *bufs):
    torch.cuda.synchronize()
    assert rc == 0, _lib().lib.kccot_last_error()
    for b in bufs:
        assert b.verify() is None, b.verify()


def k_fwd(x, y, win, sigma, L=1.0, want_mse=True):
    """The forward entry point with its outputs and its workspace (exactly the queried size) between guard zones"""
    lib = _lib().lib
    B, H, T, W, C = x.shape
    nb = lib.kccot_ssim_workspace_bytes(B, H, T, W, C)
    assert 0 < nb < 1 << 20
    s, m, ws = ag.guarded(B * T * 4, "output", "ssim_out"), ag.guarded(B * T * 4, "output", "mse_out"), ag.guarded(nb, "workspace", "ws")
    gx, gy = ag.guarded_input("x", x), ag.guarded_input("y", y)
    _done(lib.kccot_ssim_fwd_f32(gx.ptr, gy.ptr, B, H, T, W, C, sigma, win // 2, L, s.ptr, m.ptr if want_mse else None, ws.ptr, nb,
                                 _lib().stream_of(x)), s, m, ws, gx, gy)
    assert torch.equal(gx.view(torch.float32, x.shape), x) and torch.equal(gy.view(torch.float32, y.shape), y)
    sv, mv = s.view(torch.float32, (B, T)), m.view(torch.float32, (B, T))
    assert not bool(ag.unwritten(sv).any())
    assert not bool(ag.unwritten(mv).any()) if want_mse else bool(ag.unwritten(mv).all())
    return sv.clone(), mv.clone()


def k_bwd(g, x, y, win, sigma, L=1.0):
    lib = _lib().lib
    B, H, T, W, C = x.shape
    nb = lib.kccot_ssim_workspace_bytes(B, H, T, W, C)
    d, ws = ag.guarded(x.numel() * 4, "output", "dy"), ag.guarded(nb, "workspace", "ws")
    _done(lib.kccot_ssim_bwd_f32(g.data_ptr(), x.data_ptr(), y.data_ptr(), B, H, T, W, C, sigma, win // 2, L, d.ptr, ws.ptr, nb,
                                 _lib().stream_of(x)), d, ws)
    dv = d.view(torch.float32, x.shape)
    assert not bool(ag.unwritten(dv).any()), "dy not written everywhere"
    return dv.clone()


@pytest.fixture(scope="module")
def worst():
    w = {"ssim_noise": 0.0, "ssim_flat": 0.0, "dy": 0.0, "mse": 0.0}
    yield w
    print("\nworst over the grid: |ssim - ref| noise %.3e flat %.3e  |dy - ref| / max|ref| %.3e  |mse - ref| / ref %.3e"
          % (w["ssim_noise"], w["ssim_flat"], w["dy"], w["mse"]))


@pytest.mark.parametrize("shape,win,sigma,kind", so.GRID, ids=IDS)
def test_grid_scores_mse_and_adjoint_meet_their_bounds(shape, win, sigma, kind, worst):
    r = win // 2
    x, y = data(kind, shape, 11)
    s, m = k_fwd(x, y, win, sigma)
    xd, yd = x.double(), y.double()
    e_s = float((s.double() - so.scores(xd, yd, sigma, r)).abs().max())
    m_ref = so.mse(xd, yd)
    e_m = float(((m.double() - m_ref).abs() / m_ref).max())
    print("%s %s win %d sigma %g: |ssim - ref| %.3e  |mse - ref| / ref %.3e" % (kind, shape, win, sigma, e_s, e_m))
    worst["ssim_" + kind] = max(worst["ssim_" + kind], e_s)
    worst["mse"] = max(worst["mse"], e_m)
    e_d = None
    if kind == "noise":
        g = so.upstream(shape, 12, DEV)
        dy = k_bwd(g, x, y, win, sigma)
        ref = so.adjoint(g.double(), xd, yd, sigma, r)
        e_d = float((dy.double() - ref).abs().max()) / float(ref.abs().max())
        print("%s %s win %d sigma %g: |dy - ref| / max|ref| %.3e" % (kind, shape, win, sigma, e_d))
        worst["dy"] = max(worst["dy"], e_d)
    assert e_s <= TOL_SSIM[kind] and e_m <= TOL_MSE, (e_s, e_m)
    assert e_d is None or e_d <= TOL_DY, e_d
    # a NULL mse_out: the same scores, nothing else written
    s2, _ = k_fwd(x, y, win, sigma, want_mse=False)
    assert ag.same_bits(s, s2)


def test_another_data_range_scales_the_constants():
    shape, win, sigma, L = (2, 16, 4, 16, 2), 7, 1.5, 255.0
    x, y = data("noise", shape, 21)
    x, y = (x * L).contiguous(), (y * L).contiguous()
    s, m = k_fwd(x, y, win, sigma, L)
    g = so.upstream(shape, 22, DEV)
    dy = k_bwd(g, x, y, win, sigma, L)
    xd, yd = x.double(), y.double()
    ref = so.adjoint(g.double(), xd, yd, sigma, win // 2, L)
    assert float((s.double() - so.scores(xd, yd, sigma, win // 2, L)).abs().max()) <= TOL_SSIM["noise"]
    assert float(((m.double() - so.mse(xd, yd)).abs() / so.mse(xd, yd)).max()) <= TOL_MSE
    assert float((dy.double() - ref).abs().max()) <= TOL_DY * float(ref.abs().max())


TILED = [((1, 13, 2, 100, 3), 11), ((1, 12, 2, 20, 20), 3)]      # more than one column tile / channel tile both ways


@pytest.mark.parametrize("shape,win", [((2, 8, 3, 9, 1), 3), ((1, 13, 2, 70, 3), 11), ((1, 70, 2, 13, 2), 11)] + TILED)
def test_identical_videos_give_zero_mse_infinite_psnr_and_ssim_one(shape, win):
    from kccotgan_amd import metrics
    x, _ = data("noise", shape, 31)
    s, m = k_fwd(x, x.clone(), win, 1.5)
    assert bool((m == 0.0).all()), "mse of identical videos is exactly 0"
    assert float((s - 1.0).abs().max()) <= TOL_SSIM["noise"]
    p = metrics.psnr(x, x.clone())
    assert p.shape == (shape[0], shape[2]) and bool(torch.isposinf(p).all())
    sf, pf = metrics.frame_metrics(x, x.clone(), win_size=win)
    assert bool(torch.isposinf(pf).all()) and ag.same_bits(sf, s)


@pytest.mark.parametrize("shape,win,sigma,kind", [so.GRID[k] for k in (0, 2, 3, 6, 8, 9)], ids=[IDS[k] for k in (0, 2, 3, 6, 8, 9)])
def test_two_identical_calls_give_identical_bits(shape, win, sigma, kind):
    x, y = data(kind, shape, 41)
    g = so.upstream(shape, 42, DEV)
    s1, m1 = k_fwd(x, y, win, sigma)
    d1 = k_bwd(g, x, y, win, sigma)
    s2, m2 = k_fwd(x, y, win, sigma)
    d2 = k_bwd(g, x, y, win, sigma)
    assert ag.same_bits(s1, s2) and ag.same_bits(m1, m2) and ag.same_bits(d1, d2)


@pytest.mark.parametrize("shape,win", [((2, 8, 3, 9, 1), 3), ((2, 64, 5, 64, 1), 11), ((1, 13, 2, 70, 3), 11)] + TILED)
def test_autograd_is_the_backward_call_and_g_reaches_only_its_own_frame(shape, win):
    from kccotgan_amd import metrics
    x, y = data("noise", shape, 51)
    g = so.upstream(shape, 52, DEV)
    yv = y.clone().requires_grad_(True)
    s = metrics.ssim(x, yv, win_size=win)
    assert s.shape == (shape[0], shape[2]) and ag.same_bits(s.detach(), k_fwd(x, y, win, 1.5)[0])
    (s * g).sum().backward()
    assert ag.same_bits(yv.grad, k_bwd(g, x, y, win, 1.5))
    # one frame's g: exactly zero elsewhere, and that frame's dy is what the full g gave there scaled by nothing else
    b, t = shape[0] - 1, shape[2] - 1
    one = torch.zeros_like(g)
    one[b, t] = g[b, t]
    d1 = k_bwd(one, x, y, win, 1.5)
    mask = torch.zeros(shape, dtype=torch.bool, device=DEV)
    mask[b, :, t] = True
    assert bool((d1[~mask] == 0.0).all()) and float(d1[mask].abs().max()) > 0
    assert ag.same_bits(d1[b, :, t].contiguous(), yv.grad[b, :, t].contiguous())
    # never with respect to real
    xv = x.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="fake only"):
        metrics.ssim(xv, y, win_size=win).sum().backward()
    # 1 - SSIM as a loss term under no_grad leaves no tape
    with torch.no_grad():
        assert not metrics.ssim(x, yv, win_size=win).requires_grad


@pytest.mark.parametrize("shape", [(2, 64, 5, 64, 1), (1, 13, 2, 70, 3), (2, 8, 3, 9, 1)] + [c[0] for c in TILED])
def test_frame_metrics_equals_ssim_and_psnr_called_separately(shape):
    """bit for bit at the default window (psnr runs the walk at that window; a frame below 11 x 11: at win_size 1)"""
    from kccotgan_amd import metrics
    x, y = data("noise", shape, 61)
    win = 11 if min(shape[1], shape[3]) >= 11 else 1
    s, p = metrics.frame_metrics(x, y, win_size=win)
    assert not s.requires_grad and not p.requires_grad and s.shape == p.shape == (shape[0], shape[2])
    assert ag.same_bits(s, metrics.ssim(x, y, win_size=win)) and ag.same_bits(p, metrics.psnr(x, y))
    m = k_fwd(x, y, win, 1.5)[1]
    assert ag.same_bits(p, 10.0 * torch.log10(1.0 / m))
    # in dB: an mse within 2e-6 relative moves 10 log10 by 1e-5, fp32 log10 and its argument's rounding by a few 1e-6 at ~20 dB
    ref = 10.0 * torch.log10(1.0 / so.mse(x.double(), y.double()))
    assert float((p.double() - ref).abs().max()) <= 1e-4
    # scale invariance: both sides lie within the tolerance of one real number
    s255, p255 = metrics.frame_metrics(x * 255.0, y * 255.0, data_range=255.0, win_size=win)
    assert float((p255 - p).abs().max()) <= 1e-4 and float((s255 - s).abs().max()) <= 2 * TOL_SSIM["noise"]


def test_evaluate_is_frame_metrics_of_the_sampled_frames(monkeypatch):
    from kccotgan_amd import gan, metrics
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2          # the smallest configuration of tests/test_gpu_train_step.py
    tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="none", warmup=10,
                      device=DEV)
    test_data = torch.rand(B, H, T, W, C, device=DEV)
    torch.manual_seed(1234)
    res = tr.evaluate(test_data)
    torch.manual_seed(1234)
    video = tr.sample(test_data)
    s, p = metrics.frame_metrics(test_data[:, :, iT:].contiguous(), video[:, :, iT:].contiguous())
    assert sorted(res) == ["psnr", "ssim"]
    assert res["ssim"].shape == res["psnr"].shape == (T - iT,) == (tr.pred_time_steps,)
    assert ag.same_bits(res["ssim"], s.mean(0)) and ag.same_bits(res["psnr"], p.mean(0))
    assert bool(torch.isfinite(res["ssim"]).all()) and bool(torch.isfinite(res["psnr"]).all())
    assert not res["ssim"].requires_grad
    torch.manual_seed(1234)
    res7 = tr.evaluate(test_data, data_range=2.0, win_size=7, ssim_sigma=1.0)
    s7, p7 = metrics.frame_metrics(test_data[:, :, iT:].contiguous(), video[:, :, iT:].contiguous(), 2.0, 7, 1.0)
    assert ag.same_bits(res7["ssim"], s7.mean(0)) and ag.same_bits(res7["psnr"], p7.mean(0))
