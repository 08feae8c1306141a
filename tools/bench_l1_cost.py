#!/usr/bin/env python3
"""Kernel timing of the L1 ground cost (KCCOT_COST_L1, include/kccot_l1.h) at the configs[1] shape (B = 64, T = 30, 64 x 64 x 1:
K = 122880) and at B = 8: the L1 cost3 forward beside the squared cost3 forward forced onto the same direct-difference kernel
(KCCOT_COST_FORCE_DIRECT -- the yardstick: the same loads and LDS traffic, two VALU issues per two pairs where L1 spends three),
the default squared path for context, kccot_l1_cost3_bwd_f32 beside its issue floor, and the whole L1 loss, forward + backward,
through the Python API (host work included).  The two forwards are timed in alternation, batch by batch: HIP events around
back-to-back calls -- at least `reps` of them, and as many as fill a window of 0.25 s -- the median of `batches` such batches and
the batch-to-batch spread (min, max).  Cache regime: every call re-reads the same two videos (configs[1]: 2 x 31.5 MB; B = 8:
2 x 3.9 MB), which stay in the 256 MiB Infinity Cache between calls -- the regime of a training step, where the cost stage follows
the kernels that wrote them.  The floor of the backward is pairs x VALU issues per pair / (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz):
the PEAK clock, not a measured one.
Prints ONE JSON line and writes it to the output file.
usage: bench_l1_cost.py [reps [batches [out.json]]]"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from kccotgan_amd import _lib, gan_utils as G
from kccotgan_amd._lib import lib, ptr, check

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
BATCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 7
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "l1_cost_bench.json")
SHAPES = {"configs[1]": (64, 64, 30, 64, 1), "B=8": (8, 64, 30, 64, 1)}
T, J, SC = 30, 8, 1.0 / 15.0
WINDOW_S = 0.25
LANES, PEAK_HZ = 256 * 4 * 16, 2.4e9
BWD_ISSUES_PER_PAIR = 4.5       # the emitted loop: 2 v_cmp + 2 v_cndmask per pair, one v_pk_fma_f32 per two pairs
FWD_RATIO_LIMIT = 1.5 * 1.10    # three issues per two pairs against two, and 10 % of run-to-run spread


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


result = {"tool": "bench_l1_cost", "min_reps": REPS, "window_s": WINDOW_S, "batches": BATCHES, "device": torch.cuda.get_device_name(0),
          "cache_regime": "inputs resident in the Infinity Cache (the same tensors every call)", "floor_clock_hz": PEAK_HZ,
          "bwd_valu_issues_per_pair": BWD_ISSUES_PER_PAIR, "fwd_ratio_limit": FWD_RATIO_LIMIT, "shapes": {}}
ok = True
for name, shape in SHAPES.items():
    B = shape[0]
    gen = torch.Generator().manual_seed(5)
    real = torch.rand(shape, generator=gen).cuda()
    fake = torch.rand(shape, generator=gen).cuda()
    fake[:, :, :10] = real[:, :, :10]                       # the trainer's fake = cat(real_in, fake_pred)
    feats = [(torch.rand((B, T, J), generator=gen) - 0.5).cuda() for _ in range(4)]
    g3 = (torch.rand((3, B, B), generator=gen) - 0.5).cuda()
    r2, f2 = real.view(B, -1), fake.view(B, -1)
    K = r2.shape[1]
    C3, dfake = torch.empty((3, B, B), device="cuda"), torch.empty_like(f2)
    wsb = int(lib.kccot_pairwise_cost3_workspace_bytes(B, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    wbb = int(lib.kccot_l1_cost3_bwd_workspace_bytes(B))
    wb = torch.empty(wbb, dtype=torch.uint8, device="cuda")
    fp = [ptr(t) for t in feats]

    def fwd(flags):
        def run():
            check(lib.kccot_pairwise_cost3_f32(ptr(r2), ptr(f2), B, K, SC, *fp, T, J, flags, ptr(C3), ws.data_ptr(), wsb, None), "cost3")
        return run

    def bwd():
        check(lib.kccot_l1_cost3_bwd_f32(ptr(g3), ptr(r2), ptr(f2), B, K, SC, ptr(dfake), wb.data_ptr(), wbb, None), "l1_cost3_bwd")

    leaves = [fake.clone().requires_grad_(True)] + [t.clone().requires_grad_(True) for t in feats]

    def loss():
        hf, hr, mr, mf = leaves[1:]
        v = G.compute_sinkhorn_loss(real, leaves[0], SC, 0.8, 100, hf, mr, hr, mf, ground_cost="l1")
        torch.autograd.grad(v, leaves)

    t_l1, t_l2d = timed(fwd(_lib.COST_L1), fwd(_lib.COST_FORCE_DIRECT))
    t_l2, = timed(fwd(0))
    t_bwd, = timed(bwd)
    t_loss, = timed(loss)
    pairs = B * 2 * B * K
    floor_us = pairs * BWD_ISSUES_PER_PAIR / (LANES * PEAK_HZ) * 1e6
    ratio = t_l1["us"] / t_l2d["us"]
    ok = ok and ratio <= FWD_RATIO_LIMIT
    row = {"shape": list(shape), "K": K, "fwd_l1": t_l1, "fwd_l2_forced_direct": t_l2d, "fwd_l2_default_path": t_l2,
           "ratio_fwd_l1_over_l2_forced_direct": round(ratio, 3), "bwd_l1_cost3": t_bwd, "bwd_pairs": pairs,
           "bwd_issue_floor_us": round(floor_us, 2), "bwd_over_floor": round(t_bwd["us"] / floor_us, 2),
           "bwd_source_bytes_read": 2 * B * K * 4 * ((B + 7) // 8), "loss_l1_fwd_plus_bwd_python": t_loss}
    result["shapes"][name] = row
    print("%s: fwd L1 %.1f us, squared forced direct %.1f us (ratio %.3f, limit %.2f), squared default path %.1f us; L1 bwd %.1f us "
          "(%.3g pairs, issue floor %.1f us: %.2f x); L1 loss fwd + bwd %.1f us" % (name, t_l1["us"], t_l2d["us"], ratio, FWD_RATIO_LIMIT,
                                                                                  t_l2["us"], t_bwd["us"], pairs, floor_us,
                                                                                  t_bwd["us"] / floor_us, t_loss["us"]), flush=True)
    del real, fake, feats, g3, C3, dfake, ws, wb, leaves
    torch.cuda.empty_cache()
result["fwd_ratio_within_limit"] = ok
line = json.dumps(result)
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as fh:
    fh.write(line + "\n")
print(line)
sys.exit(0 if ok else 1)
