#!/usr/bin/env python3
"""Timing of the batch-sharded bi-causal loss at world size 1 over RCCL (one GPU), option sinkhorn_shortcut = 0 (every
Sinkhorn iteration executes).  Prints ONE JSON line:
  step          graph-replayed sharded step (GraphedShardedStep: input all-gathers as RCCL calls, then the graph) at the
                configs[1] shape (B = 64, 64 x 64 frames, T = 30, J = 8), bi_causal=True against the one-batch step on the
                same inputs: ms per step (median of `--blocks` alternating blocks of `--iters` steps) and the ratio;
  phases        dist.phase_timing() of eager steps, one-batch and bi-causal, at the configs[1] shape and at B = 128, 256,
                512 on decimated frames (8 x 8, T = 30, J = 8): ms per step per phase; "bicausal_term" is the new launch;
  term_us       the KCCOT_COST_BICAUSAL_TERM_ONLY launch alone, replayed from a graph of 20 launches, per launch.
Launch: a process with MASTER_ADDR / MASTER_PORT / RANK=0 / WORLD_SIZE=1 / LOCAL_RANK=0 (or torch.distributed.run).
usage: bench_sharded_bicausal.py [--iters N] [--blocks N] [--out FILE]"""
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


def inputs(B, H, T, W, C, J, dev, seed=1234):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(B, H, T, W, C, generator=g)
    fake = (real + 0.05 * torch.randn(real.shape, generator=g)).clamp(0, 1)
    t = {"real": real, "fake": fake}
    t.update({k: torch.rand(B, T, J, generator=g) for k in ("h_fake", "m_real", "h_real", "m_fake")})
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


def phases(kd, shard, bi_causal, steps):
    kd.sharded_loss_step(shard, SC, bi_causal=bi_causal)          # warm-up: workspaces, allocator
    kd.phase_timing(True)
    for _ in range(steps):
        kd.sharded_loss_step(shard, SC, bi_causal=bi_causal)
    out = kd.phase_ms()
    kd.phase_timing(False)
    n = out.pop("steps")
    return {k: round(v / n, 5) for k, v in out.items()}


def term_us(kd, t, launches=20, iters=50):
    B = t["real"].shape[0]
    C3 = torch.zeros(3, B, B, device=t["real"].device)
    f = [t[k].float().contiguous() for k in ("h_fake", "h_real", "m_real", "m_fake")]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        kd.HipOps.bicausal_term(C3, *f, SC)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            kd.HipOps.bicausal_term(C3, *f, SC)
    for _ in range(5):
        g.replay()
    return 1e3 * time_step(g.replay, iters) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--phase-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29517"), ("RANK", "0"), ("WORLD_SIZE", "1")):
        os.environ.setdefault(k, v)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)
    from kccotgan_amd import _lib, dist as kd
    from kccotgan_amd.graph import GraphedShardedStep
    _lib.set_option("sinkhorn_shortcut", 0)
    t0 = time.time()
    res = {"world": dist.get_world_size(), "backend": dist.get_backend(), "sinkhorn_shortcut": 0, "shape": list(CFG1[:5]),
           "J": CFG1[5], "iters": args.iters, "blocks": args.blocks}
    shard = kd.shard_batch(inputs(*CFG1, dev), 0, 1)
    steps = {"one_batch": GraphedShardedStep(shard, SC), "bicausal": GraphedShardedStep(shard, SC, bi_causal=True)}
    ms = {k: [] for k in steps}
    for k, s in steps.items():
        time_step(s, 20)
    for _ in range(args.blocks):                       # alternating blocks: drift hits both alike
        for k, s in steps.items():
            ms[k].append(time_step(s, args.iters))
    res["step_ms"] = {k: round(statistics.median(v), 5) for k, v in ms.items()}
    res["step_ms_blocks"] = {k: [round(x, 5) for x in v] for k, v in ms.items()}
    res["bicausal_over_one_batch"] = round(res["step_ms"]["bicausal"] / res["step_ms"]["one_batch"], 4)
    res["bar_ratio"] = 1.05
    del steps
    res["phases_ms"], res["term_us"] = {}, {}
    for name, shape in (("B64_configs1", CFG1), ("B128_deci", (128, 8, 30, 8, 1, 8)), ("B256_deci", (256, 8, 30, 8, 1, 8)),
                        ("B512_deci", (512, 8, 30, 8, 1, 8))):
        t = inputs(*shape, dev)
        sh = kd.shard_batch(t, 0, 1)
        res["phases_ms"][name] = {"one_batch": phases(kd, sh, False, args.phase_steps),
                                  "bicausal": phases(kd, sh, True, args.phase_steps)}
        res["term_us"][name] = round(term_us(kd, t), 3)
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
