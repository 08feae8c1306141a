#!/usr/bin/env python3
"""Forward + backward of compute_conditional_sinkhorn_loss at the configs[1] shape (B = 64, 64 x 64 frames, T = 30, J = 8) for
Q in {1, 16, 64} queries, through the Python API with eager launches, event-timed call by call, next to -- in the same process,
on the same inputs --
  * compute_weighted_sinkhorn_loss (one weighted loss: the floor a single query cannot beat), and
  * the composition the library offered before the conditional entry points: C3 assembled once, copied Q times into a
    [3Q,B,B] tensor, the weighted solver on the copy, the combination sum_q omega_q (2 c_q0 - c_q1 - c_q2) in torch (autograd
    then sums the Q gradients).  It exists only here, since the library has no function for it.
All run epsilon = 0.8, L = 100 with option sinkhorn_shortcut = 0, so that every Sinkhorn iteration runs and the timing does
not depend on the inputs becoming periodic.  Prints ONE JSON line.
usage: bench_conditional_loss.py [--iters N] [--warmup N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from kccotgan_amd import _lib, gan_utils as G  # noqa: E402

EPS, LIT, SC = 0.8, 100, 1 / 15.0


def times_ms(fn, iters, warmup):
    """p10 / p50 / p90 / mean of `iters` eager calls, one event pair each, after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
    pick = lambda q: t[min(len(t) - 1, int(q * len(t)))]
    return {"p10": pick(0.10), "p50": pick(0.50), "p90": pick(0.90), "mean": sum(t) / len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
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
    # the weights a trainer would use: the kernel estimate given each sample's first 10 frames, per-pixel RMS bandwidth 0.2
    ctx = real[:, :, :10].contiguous()
    weights = G.kernel_conditional_weights(ctx, 0.2 * (ctx[0].numel() ** 0.5))
    coef = torch.tensor([2.0, -1.0, -1.0], device="cuda")
    flat = lambda v: v.reshape(B, -1)

    def conditional(w):
        loss = G.compute_conditional_sinkhorn_loss(real, fake, SC, EPS, LIT, f["h_fake"], f["m_real"], f["h_real"], f["m_fake"], w)
        return torch.autograd.grad(loss, wrt)

    def weighted():
        loss = G.compute_weighted_sinkhorn_loss(real, fake, SC, EPS, LIT, f["h_fake"], f["m_real"], f["h_real"], f["m_fake"],
                                                weights[0], weights[0], normalize=False)
        return torch.autograd.grad(loss, wrt)

    def composition(w):
        Q = w.shape[0]
        C3 = G._Cost3.apply(flat(real), flat(fake), f["h_fake"], f["h_real"], f["m_real"], f["m_fake"], SC)
        wx = w.repeat_interleave(3, dim=0).contiguous()
        costs = G._WeightedSinkhorn.apply(C3.repeat(Q, 1, 1), wx, wx, EPS, LIT, 100, _lib.STOP_COUNT, "bench_composition")
        loss = (costs.view(Q, 3) * coef).sum() / Q
        return torch.autograd.grad(loss, wrt)

    res = {"shape": [B, H, T, W, C], "J": J, "iters": args.iters, "warmup": args.warmup, "sinkhorn_shortcut": 0, "eps": EPS,
           "L": LIT, "launches": "eager", "rows": {}}
    t0 = time.time()
    res["rows"]["weighted_loss"] = times_ms(weighted, args.iters, args.warmup)
    for Q in (1, 16, 64):
        w = weights[:Q].contiguous()
        a, b = conditional(w), composition(w)                       # the two paths compute the same thing
        res["rows"]["conditional_Q%d" % Q] = times_ms(lambda: conditional(w), args.iters, args.warmup)
        res["rows"]["composition_Q%d" % Q] = times_ms(lambda: composition(w), args.iters, args.warmup)
        res["max_rel_gap_dfake_Q%d" % Q] = float((a[0] - b[0]).abs().max() / b[0].abs().max())
    res["rows"]["weighted_loss_again"] = times_ms(weighted, args.iters, args.warmup)
    r = res["rows"]
    res["conditional_Q64_p50_below_composition_Q64_p10"] = bool(r["conditional_Q64"]["p50"] < r["composition_Q64"]["p10"])
    res["conditional_Q64_over_weighted_p50"] = r["conditional_Q64"]["p50"] / r["weighted_loss"]["p50"]
    res["conditional_Q1_over_weighted_p50"] = r["conditional_Q1"]["p50"] / r["weighted_loss"]["p50"]
    res["path"] = G.last_info["compute_conditional_sinkhorn_loss_path"]
    res["wall_s"] = time.time() - t0
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
