#!/usr/bin/env python3
"""Kernel timing of the sliced Wasserstein distance (include/kccot_swd.h) at the configs[1] shape (B = 64, T = 30, 64 x 64 x 1:
K = 122880) and at B = 8, with P = 128 projections: kccot_swd_fwd_f32 (three launches) and kccot_swd_bwd_f32 (dfake alone, and
dreal + dfake), beside three figures:
  - the algorithmic floor of the forward, max(bytes / HBM rate, 2 * 2B * K * P / fp32-matrix peak) with the two videos as the
    bytes (peaks of the data sheet: 8 TB/s, 157.3 TFLOP/s; which of the two bounds is named);
  - the time of kccot_swd_directions_f32 for the same P x K elements: the generator alone, with one 4-byte store per element that
    the fused kernels do not pay -- an upper estimate of the generation share;
  - the same value by stock torch with the directions ALREADY in memory and already normalised (two matmuls against a resident
    [P,K] matrix, two sorts, the mean of the squared differences): the yardstick.  It reads twice the bytes and gets its
    directions for free; the fused forward must not be slower (margin 1.0), and the tool exits 1 if it is.
The fused forward and the yardstick are timed in alternation, batch by batch: HIP events around back-to-back calls -- at least
`reps` of them, and as many as fill a window of 0.25 s -- the median of `batches` such batches and the batch-to-batch spread
(min, max).  Cache regime: every call re-reads the same two videos (configs[1]: 2 x 31.5 MB; B = 8: 2 x 3.9 MB) and, for the
yardstick, the same 63 MB of directions; all of it stays in the 256 MiB Infinity Cache between calls -- the regime of a monitor
that follows the kernels which wrote the videos.
Prints ONE JSON line and writes it to the output file.
usage: bench_swd.py [reps [batches [out.json]]]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kccotgan_amd import _lib
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "swd_bench.json")
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "B=8": (8, 64, 30, 64, 1)}
P, SEED = 128, 0
WINDOW_S = 0.25
HBM_BYTES_S, F32_MATRIX_FLOPS = 8.0e12, 157.3e12
MARGIN = 1.0


def batch_us(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def timed(*fns):
    """the functions in alternation, batch by batch"""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    reps = [max(REPS, int(WINDOW_S * 1e6 / batch_us(f, REPS)) + 1) for f in fns]
    us = [[] for _ in fns]
    for _ in range(BATCHES):
        for k, f in enumerate(fns):
            us[k].append(batch_us(f, reps[k]))
    return [{"us": round(statistics.median(u), 2), "us_min_max": [round(min(u), 2), round(max(u), 2)], "calls_per_batch": r}
            for u, r in zip(us, reps)]


result = {"tool": "bench_swd", "min_reps": REPS, "window_s": WINDOW_S, "batches": BATCHES, "device": torch.cuda.get_device_name(0),
          "cache_regime": "inputs (and the yardstick's directions) resident in the Infinity Cache (the same tensors every call)",
          "P": P, "hbm_bytes_per_s": HBM_BYTES_S, "f32_matrix_flops": F32_MATRIX_FLOPS, "margin": MARGIN, "shapes": {}}
ok = True
for name, shape in SHAPES.items():
    B = shape[0]
    gen = torch.Generator().manual_seed(5)
    real = torch.rand(shape, generator=gen).cuda().view(B, -1)
    fake = (real + 0.05 * torch.randn(real.shape, generator=gen).cuda()).clamp_(0, 1)
    K = real.shape[1]
    plan = _lib.swd_plan(B, K, P)
    proj, order = torch.empty((2, P, B), device="cuda"), torch.empty((2, P, B), dtype=torch.int32, device="cuda")
    inv, out, g = torch.empty(P, device="cuda"), torch.empty(1, device="cuda"), torch.ones(1, device="cuda")
    dreal, dfake = torch.empty_like(real), torch.empty_like(fake)
    wsb = int(lib.kccot_swd_workspace_bytes(B, K, P))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    theta = torch.empty((P, K), device="cuda")
    check(lib.kccot_swd_directions_f32(SEED, K, 0, P, ptr(theta), None), "swd_directions")
    unit_t = (theta / theta.norm(dim=1, keepdim=True)).t().contiguous()          # [K,P], resident: the yardstick's free input

    def fwd():
        check(lib.kccot_swd_fwd_f32(ptr(real), ptr(fake), B, K, P, SEED, ptr(proj), ptr(order), ptr(inv), ptr(out), ws.data_ptr(), wsb,
                                    None), "swd_fwd")

    def torch_fwd():
        d = torch.sort(real @ unit_t, dim=0)[0] - torch.sort(fake @ unit_t, dim=0)[0]
        return (d * d).mean()

    def bwd(want_real):
        def run():
            check(lib.kccot_swd_bwd_f32(ptr(g), ptr(proj), ptr(order), ptr(inv), B, K, P, SEED, ptr(dreal) if want_real else None,
                                        ptr(dfake), ws.data_ptr(), wsb, None), "swd_bwd")
        return run

    def directions():
        check(lib.kccot_swd_directions_f32(SEED, K, 0, P, ptr(theta), None), "swd_directions")

    fwd()
    v_fused, v_torch = float(out), float(torch_fwd())
    t_fwd, t_torch = timed(fwd, torch_fwd)
    t_bwd_fake, = timed(bwd(False))
    t_bwd_both, = timed(bwd(True))
    t_dir, = timed(directions)
    bytes_us = 2 * B * K * 4 / HBM_BYTES_S * 1e6
    flops_us = 2.0 * 2 * B * K * P / F32_MATRIX_FLOPS * 1e6
    floor_us = max(bytes_us, flops_us)
    ratio = t_fwd["us"] / t_torch["us"]
    ok = ok and ratio <= MARGIN
    row = {"shape": list(shape), "K": K, "plan": plan, "workspace_bytes": wsb, "fwd": t_fwd, "fwd_stock_torch_resident_directions": t_torch,
           "ratio_fwd_over_stock_torch": round(ratio, 3), "fwd_floor_us": round(floor_us, 2),
           "fwd_floor_bound": "fp32 matrix" if flops_us >= bytes_us else "HBM bytes", "fwd_over_floor": round(t_fwd["us"] / floor_us, 2),
           "directions_call": t_dir, "directions_call_over_fwd": round(t_dir["us"] / t_fwd["us"], 3), "bwd_dfake": t_bwd_fake,
           "bwd_dreal_dfake": t_bwd_both, "sw2_fused": v_fused, "sw2_stock_torch": v_torch}
    result["shapes"][name] = row
    print("%s: fwd %.1f us, stock torch with resident directions %.1f us (ratio %.3f, margin %.1f); floor %.1f us (%s): %.2f x; "
          "directions call %.1f us (%.2f of fwd); bwd dfake %.1f us, dreal + dfake %.1f us; SW2 %.6e (torch %.6e)"
          % (name, t_fwd["us"], t_torch["us"], ratio, MARGIN, floor_us, row["fwd_floor_bound"], t_fwd["us"] / floor_us, t_dir["us"],
             t_dir["us"] / t_fwd["us"], t_bwd_fake["us"], t_bwd_both["us"], v_fused, v_torch), flush=True)
    del real, fake, proj, order, dreal, dfake, ws, theta, unit_t
    torch.cuda.empty_cache()
result["fwd_within_margin"] = ok
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
print(line)
sys.exit(0 if ok else 1)
