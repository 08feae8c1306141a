#!/usr/bin/env python3
"""Forward + backward of compute_bicausal_sinkhorn_loss at the configs[1] shape (B = 64, 64 x 64 frames, T = 30, J = 8),
replayed from a graph, next to compute_sinkhorn_loss on the same inputs.  Option sinkhorn_shortcut = 0 so that every
Sinkhorn iteration runs (the timing does not depend on the inputs becoming periodic).  Prints ONE JSON line.
usage: bench_bicausal_loss.py [--iters N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from kccotgan_amd import _lib, gan_utils as G  # noqa: E402


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def time_ms(g, iters):
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(iters):
        g.replay()
    ev1.record()
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.set_option("sinkhorn_shortcut", 0)
    B, H, T, W, C, J = 64, 64, 30, 64, 1, 8
    gen = torch.Generator(device="cpu").manual_seed(1234)
    rnd = lambda *s: torch.rand(*s, generator=gen).cuda()
    real = rnd(B, H, T, W, C)
    fake = (real + 0.05 * torch.randn(real.shape, generator=gen).cuda()).clamp(0, 1).requires_grad_(True)
    f = {k: rnd(B, T, J).requires_grad_(True) for k in ("h_fake", "m_real", "h_real", "m_fake")}
    wrt = [fake] + [f[k] for k in ("h_fake", "h_real", "m_real", "m_fake")]

    def bicausal_fwd():
        return G.compute_bicausal_sinkhorn_loss(real, fake, 1 / 15.0, 0.8, 100, f["h_fake"], f["m_real"], f["h_real"],
                                                f["m_fake"])

    def one_fwd():
        return G.compute_sinkhorn_loss(real, fake, 1 / 15.0, 0.8, 100, f["h_fake"], f["m_real"], f["h_real"], f["m_fake"])

    res = {"shape": [B, H, T, W, C], "J": J, "iters": args.iters, "sinkhorn_shortcut": 0}
    t0 = time.time()
    for name, fwd in (("bicausal", bicausal_fwd), ("one_batch", one_fwd)):
        res[name + "_fwd_bwd_ms"] = time_ms(graphed(lambda: torch.autograd.grad(fwd(), wrt)), args.iters)
        with torch.no_grad():
            res[name + "_fwd_only_ms"] = time_ms(graphed(fwd), args.iters)
    res["bicausal_fused_sweep"] = bool(G.last_info.get("compute_bicausal_sinkhorn_loss_fused_sweep", False))
    res["bicausal_over_one_batch"] = res["bicausal_fwd_bwd_ms"] / res["one_batch_fwd_bwd_ms"]
    res["bar_ratio"] = 1.05
    res["wall_s"] = time.time() - t0
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
