#!/usr/bin/env python3
"""Timing of the batch-sharded RBF-kernel MMD at world size 1 over RCCL (one GPU).  Prints ONE JSON line:
  rbf_sum_us     the KCCOT_COST_RBF_SUM call alone (two launches: tiles + combine), replayed from a graph of 20 calls, per
                 call, at [Bl, B] = [64,64], [32,256], [64,512]; `three_blocks_64x512` = the three blocks of one rank at
                 B = 512 on 8 ranks, per rank;
  rbf_mmd_us     the single-GPU kernel kccot_rbf_mmd_f32 (ONE workgroup over 3 B^2 entries) on the full D3 at B = 64, 256
                 and 512, the same way, alternating blocks with the above (median of `--blocks` blocks of `--iters` replays);
  step_ms        eager forward + backward (d / d fake): dist.sharded_rbf_mmd2 at world size 1 against mmd.rbf_mmd2 on the same
                 inputs, at the configs[1] (B = 64, 64 x 64 x 1, T = 30) and configs[3] (B = 256, 64 x 64 x 3, T = 30) shapes,
                 alternating blocks, and their ratio.  At world size 1 a rank owns ALL rows: Bl = 64 / 256, the direct rows
                 kernel (the matrix-pipe row blocks serve 32 or 64 rows per rank at B % 128 == 0) -- this is the cost of the
                 protocol on one card, not a scaling figure;
  phases_ms      dist.phase_timing() of those eager sharded steps: exchange_inputs, cost_rows, mmd_rows, reduce, gradient, and
                 at B = 128, 256, 512 on decimated frames (8 x 8 x 4, T = 10; all rows on one rank: the direct kernel too).
Nothing here has run on more than one GPU.
Launch: a process with MASTER_ADDR / MASTER_PORT / RANK=0 / WORLD_SIZE=1 / LOCAL_RANK=0 (or torch.distributed.run).
usage: bench_sharded_mmd.py [--iters N] [--blocks N] [--step-iters N] [--phase-steps N] [--out FILE]"""
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

CFG1 = (64, 64, 30, 64, 1)
CFG3 = (256, 64, 30, 64, 3)


def inputs(shape, dev, seed=1234):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(shape, generator=g)
    fake = (real + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    return real.to(dev), fake.to(dev)


def time_step(step, iters):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def graphed(fn, warmup=2):
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


def dist_block(nblk, Bx, By, dev, seed):
    """nblk blocks of squared distances between random points of 2560 features scaled to gamma = 1 / 2560."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(nblk, Bx, By, generator=g) * 0.4 * 2560.0).to(dev)


def rbf_sum_graph(_lib, D, launches):
    """`launches` flagged calls per replay, cycling over the blocks of D (in place: after the first replay the entries are
    kernel values, exp of them again costs the same)."""
    lib = _lib.lib
    nblk, Bx, By = D.shape
    nd = (int(lib.kccot_pairwise_cost_workspace_bytes(Bx, By, 1)) + 7) // 8
    ws = torch.empty((nblk, nd), dtype=torch.float64, device=D.device)

    def fn():
        st = torch.cuda.current_stream().cuda_stream
        for i in range(launches):
            p = i % nblk
            _lib.check(lib.kccot_pairwise_cost_f32(None, None, Bx, By, 0, 1.0 / 2560.0, None, None, None, None, 1, 1,
                                                   _lib.COST_RBF_SUM, D[p].data_ptr(), ws[p].data_ptr(), nd * 8, st), "rbf sum")
    return graphed(fn), (D, ws)


def rbf_mmd_graph(_lib, B, dev, launches):
    lib = _lib.lib
    D3 = dist_block(3, B, B, dev, B)
    K3, m = torch.empty_like(D3), torch.empty(1, device=dev)

    def fn():
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(launches):
            _lib.check(lib.kccot_rbf_mmd_f32(D3.data_ptr(), B, 1.0 / 2560.0, K3.data_ptr(), m.data_ptr(), st), "rbf_mmd")
    return graphed(fn), (D3, K3, m)


def eager_steps(kd, mmd, real, fake):
    y = fake.clone().requires_grad_(True)

    def sharded():
        torch.autograd.grad(kd.sharded_rbf_mmd2(real, y), y)

    def single():
        torch.autograd.grad(mmd.rbf_mmd2(real, y), y)
    return {"single_gpu": single, "sharded": sharded}


def phases(kd, step, steps):
    step()
    kd.phase_timing(True)
    for _ in range(steps):
        step()
    out = kd.phase_ms()
    kd.phase_timing(False)
    n = out.pop("steps")
    return {k: round(v / n, 5) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--phase-steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for k, v in (("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29525"), ("RANK", "0"), ("WORLD_SIZE", "1")):
        os.environ.setdefault(k, v)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", device_id=dev)
    from kccotgan_amd import _lib, dist as kd, mmd
    t0 = time.time()
    res = {"world": dist.get_world_size(), "backend": dist.get_backend(), "iters": args.iters, "blocks": args.blocks,
           "launches_per_replay": 20}
    # ---- the flagged call against the one-workgroup kernel
    L = 20
    graphs = {"rbf_sum_64x64": rbf_sum_graph(_lib, dist_block(1, 64, 64, dev, 1), L),
              "rbf_sum_32x256": rbf_sum_graph(_lib, dist_block(1, 32, 256, dev, 2), L),
              "rbf_sum_64x512": rbf_sum_graph(_lib, dist_block(1, 64, 512, dev, 3), L),
              "rbf_sum_three_blocks_64x512": rbf_sum_graph(_lib, dist_block(3, 64, 512, dev, 4), 3 * L),
              "rbf_mmd_B64": rbf_mmd_graph(_lib, 64, dev, L), "rbf_mmd_B256": rbf_mmd_graph(_lib, 256, dev, L),
              "rbf_mmd_B512": rbf_mmd_graph(_lib, 512, dev, L)}
    us = {k: [] for k in graphs}
    for k, (g, _) in graphs.items():
        time_step(g.replay, 10)
    for _ in range(args.blocks):                       # alternating blocks: drift hits all alike
        for k, (g, _) in graphs.items():
            us[k].append(1e3 * time_step(g.replay, args.iters) / L)
    med = {k: round(statistics.median(v), 3) for k, v in us.items()}
    res["rbf_sum_us"] = {k[8:]: v for k, v in med.items() if k.startswith("rbf_sum_")}
    res["rbf_mmd_us"] = {k[8:]: v for k, v in med.items() if k.startswith("rbf_mmd_")}
    res["us_blocks"] = {k: [round(x, 3) for x in v] for k, v in us.items()}
    res["rank_blocks_B512_over_one_workgroup_B512"] = round(med["rbf_sum_three_blocks_64x512"] / med["rbf_mmd_B512"], 4)
    del graphs
    # ---- eager forward + backward and the phase split
    res["step_ms"], res["step_ms_blocks"], res["sharded_over_single_gpu"], res["phases_ms"] = {}, {}, {}, {}
    for name, shape in (("configs1", CFG1), ("configs3", CFG3)):
        real, fake = inputs(shape, dev)
        steps = eager_steps(kd, mmd, real, fake)
        ms = {k: [] for k in steps}
        for s in steps.values():
            time_step(s, 3)
        for _ in range(args.blocks):
            for k, s in steps.items():
                ms[k].append(time_step(s, args.step_iters))
        res["step_ms"][name] = {k: round(statistics.median(v), 5) for k, v in ms.items()}
        res["step_ms_blocks"][name] = {k: [round(x, 5) for x in v] for k, v in ms.items()}
        res["sharded_over_single_gpu"][name] = round(res["step_ms"][name]["sharded"] / res["step_ms"][name]["single_gpu"], 4)
        res["phases_ms"][name] = phases(kd, steps["sharded"], args.phase_steps)
        del real, fake, steps
        torch.cuda.empty_cache()
    for name, shape in (("B128_deci", (128, 8, 10, 8, 4)), ("B256_deci", (256, 8, 10, 8, 4)), ("B512_deci", (512, 8, 10, 8, 4))):
        real, fake = inputs(shape, dev)
        res["phases_ms"][name] = phases(kd, eager_steps(kd, mmd, real, fake)["sharded"], args.phase_steps)
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
