#!/usr/bin/env python3
"""Forward + backward of compute_weighted_sinkhorn_loss at the configs[1] shape (B = 64, 64 x 64 frames, T = 30, J = 8), replayed
from a graph and event-timed per replay, next to compute_sinkhorn_loss on the same inputs in the same process: on its non-fused
path (option sinkhorn_fused = 0: the like-for-like code, cost assembly -> three solves -> reverse sweep -> cost backward) and on
its default path (the one-launch fused solve + sweep, which is not weighted).  Both losses run epsilon = 0.8, L = 100
(honor_eps_l=True).  Option sinkhorn_shortcut = 0 so that every Sinkhorn iteration runs (the timing does not depend on the inputs
becoming periodic).  Prints ONE JSON line.
usage: bench_weighted_loss.py [--iters N] [--out FILE]"""
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


def times_ms(g, iters):
    """p10 / p50 / p90 / mean of `iters` replays, one event pair each."""
    for _ in range(20):
        g.replay()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        g.replay()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    pick = lambda q: t[min(len(t) - 1, int(q * len(t)))]
    return {"p10": pick(0.10), "p50": pick(0.50), "p90": pick(0.90), "mean": sum(t) / len(t)}


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
    w_real = torch.softmax(2.0 * torch.randn(B, generator=gen), 0).cuda()
    w_fake = torch.softmax(2.0 * torch.randn(B, generator=gen), 0).cuda()

    def weighted_fwd():
        return G.compute_weighted_sinkhorn_loss(real, fake, 1 / 15.0, 0.8, 100, f["h_fake"], f["m_real"], f["h_real"],
                                                f["m_fake"], w_real, w_fake, normalize=False)

    def one_fwd():
        return G.compute_sinkhorn_loss(real, fake, 1 / 15.0, 0.8, 100, f["h_fake"], f["m_real"], f["h_real"], f["m_fake"],
                                       honor_eps_l=True)

    res = {"shape": [B, H, T, W, C], "J": J, "iters": args.iters, "sinkhorn_shortcut": 0, "eps": 0.8, "L": 100}
    t0 = time.time()
    res["weighted_fwd_bwd_ms"] = times_ms(graphed(lambda: torch.autograd.grad(weighted_fwd(), wrt)), args.iters)
    res["weighted_path"] = G.last_info["compute_weighted_sinkhorn_loss_path"]
    res["weighted_fused_sweep"] = bool(G.last_info["compute_weighted_sinkhorn_loss_fused_sweep"])
    with _lib.options(sinkhorn_fused=0):
        res["one_batch_nonfused_fwd_bwd_ms"] = times_ms(graphed(lambda: torch.autograd.grad(one_fwd(), wrt)), args.iters)
        assert not G.last_info["compute_sinkhorn_loss_fused_sweep"]
    res["one_batch_fused_fwd_bwd_ms"] = times_ms(graphed(lambda: torch.autograd.grad(one_fwd(), wrt)), args.iters)
    res["one_batch_default_fused_sweep"] = bool(G.last_info["compute_sinkhorn_loss_fused_sweep"])
    # a second pass over the weighted loss, after the others: drift of the device between the passes shows here
    res["weighted_fwd_bwd_ms_again"] = times_ms(graphed(lambda: torch.autograd.grad(weighted_fwd(), wrt)), args.iters)
    nf = res["one_batch_nonfused_fwd_bwd_ms"]
    res["weighted_over_nonfused_p50"] = res["weighted_fwd_bwd_ms"]["p50"] / nf["p50"]
    res["nonfused_spread_p10_p90"] = (nf["p90"] - nf["p10"]) / nf["p50"]
    res["wall_s"] = time.time() - t0
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
