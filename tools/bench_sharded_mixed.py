#!/usr/bin/env python3
"""Timing of the batch-sharded mixed Sinkhorn divergence at world size 1 over RCCL (one GPU), option sinkhorn_shortcut = 0
(every Sinkhorn iteration executes).  Prints ONE JSON line:
  step           graph-replayed sharded step (GraphedShardedMixedStep: the input all-gathers as RCCL calls, then the graph)
                 at the configs[1] shape (B = 64, 64 x 64 frames, T = 30, J = 8) against the graph-replayed single-GPU
                 compute_mixed_sinkhorn_loss forward + backward on the same inputs: ms per step (median of `--blocks`
                 alternating blocks of `--iters` steps) and the ratio;
  phases         dist.phase_timing() of eager dist.sharded_mixed_loss_step calls at B = 128, 256, 512 on decimated frames
                 (8 x 8, T = 30, J = 8), and at B = 64 with KCCOT_DIST_ROW_BLOCKS=1: ms per step per phase;
  causal_add_us  the KCCOT_COST_CAUSAL_ADD launch alone, replayed from a graph of 20 launches, per launch: [Bl, B] =
                 [64, 512] at T = 48, J = 8, and the [64, 64] block of configs[1] (T = 30, J = 8).
Launch: a process with MASTER_ADDR / MASTER_PORT / RANK=0 / WORLD_SIZE=1 / LOCAL_RANK=0 (or torch.distributed.run).
usage: bench_sharded_mixed.py [--iters N] [--blocks N] [--phase-steps N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

SC = 1.0 / 15.0
CFG1 = (64, 64, 30, 64, 1, 8)
FEATS = ("h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")
WRT = ("fake", "fake_p") + FEATS


def inputs(B, H, T, W, C, J, dev, seed=1234):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for r, f in (("real", "fake"), ("real_p", "fake_p")):
        t[r] = torch.rand(B, H, T, W, C, generator=g)
        t[f] = (t[r] + 0.05 * torch.randn(t[r].shape, generator=g)).clamp(0, 1)
    t.update({k: torch.rand(B, T, J, generator=g) for k in FEATS})
    return {k: v.to(dev) for k, v in t.items()}


def time_step(step, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def graphed(fn, warmup=3):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warmup):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def single_gpu_step(t):
    """compute_mixed_sinkhorn_loss forward + backward on static copies of the inputs, captured as one graph."""
    from kccotgan_amd import gan_utils as G
    s = {k: v.clone() for k, v in t.items()}
    for k in WRT:
        s[k].requires_grad_(True)

    def fn():
        loss = G.compute_mixed_sinkhorn_loss(s["real"], s["fake"], s["real_p"], s["fake_p"], SC, 0.8, 100,
                                             *(s[k] for k in FEATS))
        return torch.autograd.grad(loss, [s[k] for k in WRT])
    return graphed(fn).replay


def phases(kd, shard, steps):
    kd.sharded_mixed_loss_step(shard, SC)                    # warm-up: workspaces, allocator
    kd.phase_timing(True)
    for _ in range(steps):
        kd.sharded_mixed_loss_step(shard, SC)
    out = kd.phase_ms()
    kd.phase_timing(False)
    n = out.pop("steps")
    return {k: round(v / n, 5) for k, v in out.items()}


def causal_add_us(kd, Bx, By, T, J, dev, launches=20, iters=50):
    g = torch.Generator().manual_seed(Bx + By + T)
    h, M = torch.rand(Bx, T, J, generator=g).to(dev), torch.rand(By, T, J, generator=g).to(dev)
    C = torch.zeros(Bx, By, device=dev)
    gr = graphed(lambda: [kd.HipOps.causal_add(C, h, M, SC) for _ in range(launches)], warmup=1)
    for _ in range(5):
        gr.replay()
    return 1e3 * time_step(gr.replay, iters) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--phase-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29521"), ("RANK", "0"), ("WORLD_SIZE", "1")):
        os.environ.setdefault(k, v)
    os.environ.pop("KCCOT_DIST_ROW_BLOCKS", None)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)
    from kccotgan_amd import _lib, dist as kd
    from kccotgan_amd.graph import GraphedShardedMixedStep
    _lib.set_option("sinkhorn_shortcut", 0)
    t0 = time.time()
    res = {"world": dist.get_world_size(), "backend": dist.get_backend(), "sinkhorn_shortcut": 0, "shape": list(CFG1[:5]),
           "J": CFG1[5], "iters": args.iters, "blocks": args.blocks}
    t = inputs(*CFG1, dev)
    shard = kd.shard_batch(t, 0, 1)
    sharded = GraphedShardedMixedStep(shard, SC)
    res["sharded_replicated"] = bool(sharded.replicated)
    steps = {"single_gpu": single_gpu_step(t), "sharded": sharded}
    ms = {k: [] for k in steps}
    for k, s in steps.items():
        time_step(s, 20)
    for _ in range(args.blocks):                       # alternating blocks: drift hits both alike
        for k, s in steps.items():
            ms[k].append(time_step(s, args.iters))
    res["step_ms"] = {k: round(statistics.median(v), 5) for k, v in ms.items()}
    res["step_ms_blocks"] = {k: [round(x, 5) for x in v] for k, v in ms.items()}
    res["sharded_over_single_gpu"] = round(res["step_ms"]["sharded"] / res["step_ms"]["single_gpu"], 4)
    res["bar_ratio"] = 1.10
    del steps, sharded
    res["phases_ms"] = {}
    os.environ["KCCOT_DIST_ROW_BLOCKS"] = "1"
    res["phases_ms"]["B64_configs1_rows"] = phases(kd, shard, args.phase_steps)
    os.environ.pop("KCCOT_DIST_ROW_BLOCKS")
    res["phases_ms"]["B64_configs1"] = phases(kd, shard, args.phase_steps)
    del t, shard
    for name, shape in (("B128_deci", (128, 8, 30, 8, 1, 8)), ("B256_deci", (256, 8, 30, 8, 1, 8)),
                        ("B512_deci", (512, 8, 30, 8, 1, 8))):
        res["phases_ms"][name] = phases(kd, kd.shard_batch(inputs(*shape, dev), 0, 1), args.phase_steps)
    res["causal_add_us"] = {"64x512_T48_J8": round(causal_add_us(kd, 64, 512, 48, 8, dev), 3),
                            "64x64_T30_J8": round(causal_add_us(kd, 64, 64, 30, 8, dev), 3)}
    res["wall_s"] = round(time.time() - t0, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
