#!/usr/bin/env python3
"""Kernel timing of the per-frame SSIM (include/kccot_metrics.h): forward (ssim and mse) and backward at the configs[1] and
configs[3] shapes, win_size 11, sigma 1.5, beside a plain tensor-op composition of the same definition on the same GPU: five
depthwise conv2d with the 11 x 11 outer product of the taps on permuted [B*T,C,H,W] copies, the pointwise formula, a mean; its
backward is autograd's with respect to the generated video (the permutes and the mse are part of what that user pays, so they are
timed).  The two are timed in alternation, batch by batch: HIP events around back-to-back calls -- at least `reps` of them, and
as many as fill a window of 0.25 s (a 70 us kernel: ~3500 calls per batch) -- the median of `batches` such batches and the
batch-to-batch spread (min, max) of each.  GB/s are over the ALGORITHMIC bytes: two tensor reads forward,
two reads and one write backward; the share of HBM bandwidth is over the 6.29 TB/s a float4 copy measures on an MI355X.
Prints ONE JSON line and writes it to the output file.
usage: bench_ssim.py [reps [batches [out.json]]]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F
from kccotgan_amd import _lib  # noqa: F401  (the package before the first CUDA call)
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ssim_bench.json")
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "configs[3]": (256, 64, 30, 64, 3)}
WIN, SIGMA, L = 11, 1.5, 1.0
HBM_COPY_BPS = 6.29e12
WINDOW_S = 0.25


def taps(sigma, r):
    """the library's taps to fp32 rounding (the comparison is about time; tests/test_gpu_ssim.py is about values)"""
    d = torch.arange(-r, r + 1, dtype=torch.float64)
    e = torch.exp(-d * d / (2.0 * sigma * sigma))
    return (e / e.sum()).float()


def composition(x, y, k2):
    """ssim [B,T] and mse [B,T] from tensor ops"""
    B, H, T, W, C = x.shape
    xp = x.permute(0, 2, 4, 1, 3).reshape(B * T, C, H, W)
    yp = y.permute(0, 2, 4, 1, 3).reshape(B * T, C, H, W)
    G = lambda v: F.conv2d(v, k2, groups=C)
    mx, my = G(xp), G(yp)
    sxx, syy, sxy = G(xp * xp) - mx * mx, G(yp * yp) - my * my, G(xp * yp) - mx * my
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    S = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    return S.mean(dim=(1, 2, 3)).reshape(B, T), ((xp - yp) ** 2).mean(dim=(1, 2, 3)).reshape(B, T)


def batch_us(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def timed_pair(a, b):
    for _ in range(3):
        a(); b()
    torch.cuda.synchronize()
    # calls per batch: from a first estimate, enough to fill the window
    ra, rb = (max(REPS, int(WINDOW_S * 1e6 / batch_us(f, REPS)) + 1) for f in (a, b))
    ua, ub = [], []
    for _ in range(BATCHES):
        ua.append(batch_us(a, ra))
        ub.append(batch_us(b, rb))
    fmt = lambda us, r: {"us": round(statistics.median(us), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)], "calls_per_batch": r}
    return fmt(ua, ra), fmt(ub, rb)


result = {"tool": "bench_ssim", "win_size": WIN, "sigma": SIGMA, "min_reps": REPS, "window_s": WINDOW_S, "batches": BATCHES,
          "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, shape in SHAPES.items():
    B, H, T, W, C = shape
    r = WIN // 2
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(shape, generator=gen).cuda()
    y = (x + 0.1 * torch.randn(shape, generator=gen).cuda()).clamp(0, 1).contiguous()
    g = torch.randn((B, T), generator=gen).cuda()
    w = taps(SIGMA, r).cuda()
    k2 = (w[:, None] * w[None, :])[None, None].repeat(C, 1, 1, 1).contiguous()
    s, m, dy = torch.empty((B, T), device="cuda"), torch.empty((B, T), device="cuda"), torch.empty_like(y)
    wsb = int(lib.kccot_ssim_workspace_bytes(*shape))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    yv = y.clone().requires_grad_(True)

    def k_fwd():
        check(lib.kccot_ssim_fwd_f32(ptr(x), ptr(y), *shape, SIGMA, r, L, ptr(s), ptr(m), ws.data_ptr(), wsb, None), "ssim_fwd")

    def k_bwd():
        check(lib.kccot_ssim_bwd_f32(ptr(g), ptr(x), ptr(y), *shape, SIGMA, r, L, ptr(dy), ws.data_ptr(), wsb, None), "ssim_bwd")

    def c_fwd():
        with torch.no_grad():
            composition(x, y, k2)

    def c_fwd_bwd():
        yv.grad = None
        (composition(x, yv, k2)[0] * g).sum().backward()

    # the two compute the same thing
    k_fwd(); k_bwd()
    cs, cm = composition(x, yv, k2)
    (cs * g).sum().backward()
    agree = {"ssim": float((cs.detach() - s).abs().max()), "mse_rel": float(((cm.detach() - m).abs() / m).max()),
             "dy_over_max": float((yv.grad - dy).abs().max() / dy.abs().max())}
    kf, cf = timed_pair(k_fwd, c_fwd)
    kb, cfb = timed_pair(k_bwd, c_fwd_bwd)
    n_bytes = x.numel() * 4
    row = {"shape": list(shape), "workspace_bytes": wsb, "agreement": agree,
           "kernel": {"fwd": kf, "bwd": kb}, "composition": {"fwd": cf, "fwd_plus_bwd": cfb}}
    for key, t, nb in (("fwd", kf, 2 * n_bytes), ("bwd", kb, 3 * n_bytes)):
        bps = nb / (t["us"] * 1e-6)
        row["kernel"][key]["algorithmic_GBps"] = round(bps / 1e9, 1)
        row["kernel"][key]["share_of_hbm_copy_bandwidth"] = round(bps / HBM_COPY_BPS, 4)
    # autograd cannot run a backward without its forward: the composition's backward is the difference
    c_bwd_us = cfb["us"] - cf["us"]
    row["composition"]["bwd_us_by_difference"] = round(c_bwd_us, 2)
    row["ratio_fwd_composition_over_kernel"] = round(cf["us"] / kf["us"], 3)
    row["ratio_bwd_composition_over_kernel"] = round(c_bwd_us / kb["us"], 3)
    row["ratio_fwd_plus_bwd_composition_over_kernel"] = round(cfb["us"] / (kf["us"] + kb["us"]), 3)
    result["shapes"][name] = row
    print("%s %s: kernel fwd %.1f us (%.0f GB/s) bwd %.1f us (%.0f GB/s); composition fwd %.1f us, fwd+bwd %.1f us; "
          "composition / kernel: fwd %.2f, fwd+bwd %.2f" % (name, shape, kf["us"], row["kernel"]["fwd"]["algorithmic_GBps"], kb["us"],
                                                          row["kernel"]["bwd"]["algorithmic_GBps"], cf["us"], cfb["us"],
                                                          row["ratio_fwd_composition_over_kernel"],
                                                          row["ratio_fwd_plus_bwd_composition_over_kernel"]), flush=True)
    del x, y, g, s, m, dy, ws, yv, cs, cm
    torch.cuda.empty_cache()
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
print(line)
