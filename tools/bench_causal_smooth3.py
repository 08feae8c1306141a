#!/usr/bin/env python3
"""Kernel-only timing of the causal 3-D smoothing (include/kccot_smooth_causal3.h) beside the symmetric 3-D call
(KCCOT_SMOOTH_T|H|W), forward and backward, in the same process at the configs[1] and configs[3] shapes with sigma = 5, r = 3:
HIP events around `reps` back-to-back calls, the median of `batches` such batches, and the batch-to-batch spread (min, max) of
each.  Both calls move the same tensors; the symmetric one is the yardstick.  Each call runs three ways: with the library's
default dispatch, with the fused walks wherever they can run (smooth_fused3 = 2) and as the chain of per-axis stages
(smooth_fused3 = 0), so that a walk that loses to its chain at a shape where the shared threshold selects it shows up.
Prints ONE JSON line and writes it to the output file.
usage: bench_causal_smooth3.py [reps [batches [out.json]]]   further options through KCCOT_OPTIONS"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kccotgan_amd import _lib
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "causal_smooth3_bench.json")
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "configs[3]": (256, 64, 30, 64, 3)}
SIGMA, RADIUS = 5.0, 3
AXES = _lib.SMOOTH_T | _lib.SMOOTH_H | _lib.SMOOTH_W


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
    return statistics.median(us), min(us), max(us)


result = {"tool": "bench_causal_smooth3", "sigma": SIGMA, "radius": RADIUS, "reps": REPS, "batches": BATCHES,
          "options": os.environ.get("KCCOT_OPTIONS", ""), "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, shape in SHAPES.items():
    x = torch.rand(shape, device="cuda")
    g = torch.randn(shape, device="cuda")
    o, din, m = torch.empty_like(x), torch.empty_like(x), torch.empty(1, device="cuda")
    wsb = int(lib.kccot_smooth_workspace_bytes(*shape))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    row = {"shape": list(shape)}
    for dispatch, opts in (("default", {}), ("walk", {"smooth_fused3": 2}), ("chain", {"smooth_fused3": 0})):
        cell = {}
        with _lib.options(**opts):
            for label, f_fwd, f_bwd, flags in (("symmetric", lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, AXES),
                                               ("causal", lib.kccot_smooth_causal3_fwd_f32, lib.kccot_smooth_causal3_bwd_f32, 0)):
                def fwd():
                    check(f_fwd(ptr(x), *shape, SIGMA, RADIUS, flags, ptr(o), ptr(m), ws.data_ptr(), wsb, None), "fwd")

                def bwd():
                    check(f_bwd(ptr(g), ptr(o), ptr(m), *shape, SIGMA, RADIUS, flags, ptr(din), ws.data_ptr(), wsb, None), "bwd")
                f = timed(fwd)
                b = timed(bwd)          # (o and m are this variant's forward output)
                cell[label] = {"fwd_us": round(f[0], 2), "fwd_us_min_max": [round(f[1], 2), round(f[2], 2)],
                               "bwd_us": round(b[0], 2), "bwd_us_min_max": [round(b[1], 2), round(b[2], 2)]}
        for k in ("fwd", "bwd"):
            s, c = cell["symmetric"], cell["causal"]
            cell[k + "_ratio_causal_over_symmetric"] = round(c[k + "_us"] / s[k + "_us"], 4)
            cell[k + "_spread_symmetric"] = round((s[k + "_us_min_max"][1] - s[k + "_us_min_max"][0]) / s[k + "_us"], 4)
            cell[k + "_spread_causal"] = round((c[k + "_us_min_max"][1] - c[k + "_us_min_max"][0]) / c[k + "_us"], 4)
        row[dispatch] = cell
    result["shapes"][name] = row
    del x, g, o, din, ws
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
print(line)
