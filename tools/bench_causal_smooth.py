#!/usr/bin/env python3
"""Kernel-only timing of the past-only temporal smoothing (KCCOT_SMOOTH_CAUSAL_T) beside the symmetric temporal call, forward
and backward, at the configs[1] and configs[3] shapes: HIP events around `reps` back-to-back calls, the median of `batches`
such batches.  Prints ONE JSON line.  Algorithmic bytes: forward 2 n 4 (read x, write out), backward 3 n 4 (read gout and out,
write din; the second read of gout and out by the two-pass statistics is not counted).
usage: bench_causal_smooth.py [reps [batches]]   options through KCCOT_OPTIONS (smooth_bwd_fold=0|1|2)"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kccotgan_amd import _lib
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "configs[3]": (256, 64, 30, 64, 3)}
SIGMA, RADIUS = 5.0, 3


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


result = {"tool": "bench_causal_smooth", "sigma": SIGMA, "radius": RADIUS, "reps": REPS, "batches": BATCHES,
          "options": os.environ.get("KCCOT_OPTIONS", ""), "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, shape in SHAPES.items():
    x = torch.rand(shape, device="cuda")
    g = torch.randn(shape, device="cuda")
    o, din, m = torch.empty_like(x), torch.empty_like(x), torch.empty(1, device="cuda")
    wsb = int(lib.kccot_smooth_workspace_bytes(*shape))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    n = x.numel()
    row = {"shape": list(shape), "fwd_bytes": 8 * n, "bwd_bytes": 12 * n}
    for label, flags in (("symmetric", _lib.SMOOTH_T), ("causal", _lib.SMOOTH_T | _lib.SMOOTH_CAUSAL_T)):
        def fwd():
            check(lib.kccot_smooth_fwd_f32(ptr(x), *shape, SIGMA, RADIUS, flags, ptr(o), ptr(m), ws.data_ptr(), wsb, None), "fwd")

        def bwd():
            check(lib.kccot_smooth_bwd_f32(ptr(g), ptr(o), ptr(m), *shape, SIGMA, RADIUS, flags, ptr(din), ws.data_ptr(), wsb,
                                           None), "bwd")
        f = timed(fwd)
        b = timed(bwd)          # (o and m are this variant's forward output)
        row[label] = {"fwd_us": round(f[0], 2), "fwd_us_min_max": [round(f[1], 2), round(f[2], 2)],
                      "fwd_TBps": round(8.0 * n / f[0] / 1e6, 3),
                      "bwd_us": round(b[0], 2), "bwd_us_min_max": [round(b[1], 2), round(b[2], 2)],
                      "bwd_TBps": round(12.0 * n / b[0] / 1e6, 3)}
    result["shapes"][name] = row
    del x, g, o, din, ws
print(json.dumps(result))
