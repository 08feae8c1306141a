#!/usr/bin/env python3
"""Kernel-only timing of the anisotropic 3-D kernel smoothing (include/kccot_smooth_aniso.h): forward, backward and the two
bandwidth gradients at the configs[1] and configs[3] shapes, sigma = (1.3, 5), r = (3, 3) and (2, 4), symmetric and causal T,
beside the isotropic entry points in the same process (kccot_smooth_fwd_f32 / _bwd_f32 with T|H|W, kccot_smooth_causal3_* for
the causal form, kccot_smooth_dsigma_f32; sigma = 5, r = 3: the yardstick -- at r = (3, 3) both move the same bytes).  HIP events
around `reps` back-to-back calls, the median of `batches` such batches and the batch-to-batch spread (min, max) of each.
Prints ONE JSON line and writes it to the output file.
usage: bench_aniso_smooth.py [reps [batches [out.json]]]   further options through KCCOT_OPTIONS"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kccotgan_amd import _lib
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "aniso_smooth_bench.json")
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "configs[3]": (256, 64, 30, 64, 3)}
SIGMA_T, SIGMA_S = 1.3, 5.0
RADII = [(3, 3), (2, 4)]
ISO_SIGMA, ISO_RADIUS = 5.0, 3
T, H, W, CT = _lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W, _lib.SMOOTH_CAUSAL_T


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


result = {"tool": "bench_aniso_smooth", "sigma": [SIGMA_T, SIGMA_S], "iso_sigma": ISO_SIGMA, "iso_radius": ISO_RADIUS, "reps": REPS,
          "batches": BATCHES, "options": os.environ.get("KCCOT_OPTIONS", ""), "device": torch.cuda.get_device_name(0), "shapes": {}}
for name, shape in SHAPES.items():
    x = torch.rand(shape, device="cuda")
    g = torch.randn(shape, device="cuda")
    o, din, m = torch.empty_like(x), torch.empty_like(x), torch.empty(1, device="cuda")
    res = torch.empty(2, device="cuda")
    wsb = int(lib.kccot_smooth_workspace_bytes(*shape))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    dwsb = int(lib.kccot_smooth_dsigma_workspace_bytes(*shape))
    dws = torch.empty(dwsb, dtype=torch.uint8, device="cuda")
    awsb = int(lib.kccot_smooth_aniso_workspace_bytes(*shape))
    aws = torch.empty(awsb, dtype=torch.uint8, device="cuda")
    row = {"shape": list(shape), "aniso_workspace_bytes": awsb}
    for causal in (False, True):
        form = "causal" if causal else "symmetric"
        i_fwd, i_bwd, iflags = ((lib.kccot_smooth_causal3_fwd_f32, lib.kccot_smooth_causal3_bwd_f32, 0) if causal else
                                (lib.kccot_smooth_fwd_f32, lib.kccot_smooth_bwd_f32, T | H | W))
        dflags = T | H | W | (CT if causal else 0)

        def iso_fwd():
            check(i_fwd(ptr(x), *shape, ISO_SIGMA, ISO_RADIUS, iflags, ptr(o), ptr(m), ws.data_ptr(), wsb, None), "fwd")

        def iso_bwd():
            check(i_bwd(ptr(g), ptr(o), ptr(m), *shape, ISO_SIGMA, ISO_RADIUS, iflags, ptr(din), ws.data_ptr(), wsb, None), "bwd")

        def iso_dsig():
            check(lib.kccot_smooth_dsigma_f32(ptr(x), ptr(g), ptr(o), ptr(m), None, *shape, ISO_SIGMA, ISO_RADIUS, dflags,
                                              ptr(res), dws.data_ptr(), dwsb, None), "dsigma")
        iso_fwd()
        cell = {"isotropic": {"fwd": timed(iso_fwd), "bwd": timed(iso_bwd), "dsigma": timed(iso_dsig)}}
        aflags = CT if causal else 0
        for rt, rs in RADII:
            cfg = (SIGMA_T, rt, SIGMA_S, rs, aflags)

            def fwd():
                check(lib.kccot_smooth_aniso_fwd_f32(ptr(x), *shape, *cfg, ptr(o), ptr(m), aws.data_ptr(), awsb, None), "fwd")

            def bwd():
                check(lib.kccot_smooth_aniso_bwd_f32(ptr(g), ptr(o), ptr(m), *shape, *cfg, ptr(din), aws.data_ptr(), awsb, None),
                      "bwd")

            def dsig():
                check(lib.kccot_smooth_aniso_dsigma_f32(ptr(x), ptr(g), ptr(o), ptr(m), None, *shape, *cfg, ptr(res),
                                                        aws.data_ptr(), awsb, None), "dsigma")
            fwd()
            sub = {"fwd": timed(fwd), "bwd": timed(bwd), "dsigma": timed(dsig)}
            for k in ("fwd", "bwd", "dsigma"):
                sub["ratio_%s_over_isotropic" % k] = round(sub[k]["us"] / cell["isotropic"][k]["us"], 4)
            sub["dsigma_value"] = [float(res[0]), float(res[1])]
            cell["r=(%d,%d)" % (rt, rs)] = sub
        row[form] = cell
    result["shapes"][name] = row
    del x, g, o, din, ws, dws, aws
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
print(line)
