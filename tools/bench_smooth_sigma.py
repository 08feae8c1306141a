#!/usr/bin/env python3
"""Kernel-only timing of the sigma gradient of the kernel smoothing (kccot_smooth_dsigma_f32, include/kccot_smooth_sigma.h)
beside the existing adjoint (kccot_smooth_bwd_f32, kccot_smooth_causal3_bwd_f32) of the same form, in the same process at the
configs[1] and configs[3] shapes with sigma = 5, r = 3: HIP events around `reps` back-to-back calls, the median of `batches`
such batches and the batch-to-batch spread (min, max) of each.  Both move three tensors (dsigma reads three, the adjoint reads
two and writes one); the adjoint is the yardstick.  The sigma gradient runs twice: with stats_in = NULL (it takes the two sums
of the normalisation's adjoint itself: one more pass over gout and out) and with the sums handed in (the sharded protocol).
Prints ONE JSON line and writes it to the output file.
usage: bench_smooth_sigma.py [reps [batches [out.json]]]   further options through KCCOT_OPTIONS"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kccotgan_amd import _lib
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "smooth_sigma_bench.json")
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "configs[3]": (256, 64, 30, 64, 3)}
SIGMA, RADIUS = 5.0, 3
T, H, W, CT = _lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W, _lib.SMOOTH_CAUSAL_T
# form -> (forward, adjoint, the flags of those two, axes_flags of the sigma gradient)
FORMS = {"T": (lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, T, T),
         "causal T": (lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, T | CT, T | CT),
         "H|W": (lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, H | W, H | W),
         "T|H|W": (lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, T | H | W, T | H | W),
         "causal T|H|W": (lib.kccot_smooth_causal3_fwd_f32, lib.kccot_smooth_causal3_bwd_f32, 0, T | H | W | CT)}


def timed(run):
    for _ in range(5):
        run()
    torch.cuda.synchronize()
    us = []
    for _ in range(BATCHES):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            run()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / REPS * 1e3)
    return {"us": round(statistics.median(us), 2), "us_min_max": [round(min(us), 2), round(max(us), 2)]}


result = {"tool": "bench_smooth_sigma", "sigma": SIGMA, "radius": RADIUS, "reps": REPS, "batches": BATCHES,
          "options": os.environ.get("KCCOT_OPTIONS", ""), "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, shape in SHAPES.items():
    x = torch.rand(shape, device="cuda")
    g = torch.randn(shape, device="cuda")
    o, din, m = torch.empty_like(x), torch.empty_like(x), torch.empty(1, device="cuda")
    stats, res = torch.zeros(2, device="cuda"), torch.empty(1, device="cuda")
    wsb = int(lib.kccot_smooth_workspace_bytes(*shape))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dwsb = int(lib.kccot_smooth_dsigma_workspace_bytes(*shape))
    dws = torch.empty(dwsb, dtype=torch.uint8, device="cuda")
    row = {"shape": list(shape), "dsigma_workspace_bytes": dwsb}
    for label, (f_fwd, f_bwd, flags, dflags) in FORMS.items():
        check(f_fwd(ptr(x), *shape, SIGMA, RADIUS, flags, ptr(o), ptr(m), ws.data_ptr(), wsb, None), "fwd")
        stats[0] = (g.double() * o.double()).sum().float()
        stats[1] = (o == 1.0).sum().float()

        def bwd():
            check(f_bwd(ptr(g), ptr(o), ptr(m), *shape, SIGMA, RADIUS, flags, ptr(din), ws.data_ptr(), wsb, None), "bwd")

        def dsig():
            check(lib.kccot_smooth_dsigma_f32(ptr(x), ptr(g), ptr(o), ptr(m), None, *shape, SIGMA, RADIUS, dflags, ptr(res),
                                              dws.data_ptr(), dwsb, None), "dsigma")

        def dsig_stats():
            check(lib.kccot_smooth_dsigma_f32(ptr(x), ptr(g), ptr(o), ptr(m), ptr(stats), *shape, SIGMA, RADIUS, dflags, ptr(res),
                                              dws.data_ptr(), dwsb, None), "dsigma")
        cell = {"bwd": timed(bwd), "dsigma": timed(dsig), "dsigma_stats_in": timed(dsig_stats)}
        cell["ratio_dsigma_over_bwd"] = round(cell["dsigma"]["us"] / cell["bwd"]["us"], 4)
        cell["ratio_dsigma_stats_in_over_bwd"] = round(cell["dsigma_stats_in"]["us"] / cell["bwd"]["us"], 4)
        cell["dsigma_value"] = float(res)
        row[label] = cell
    result["shapes"][name] = row
    del x, g, o, din, ws, dws
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
print(line)
