#!/usr/bin/env python3
"""Backward of the conditional Sinkhorn loss (B = 64, Q = 64 queries) and of the weighted loss (B = 64) WITH and WITHOUT the
weight gradients of include/kccot_weight_grad.h, through the C ABI, event-timed call by call in one process on one forward:
  * kccot_conditional_sinkhorn_loss_bwd_f32      (what the library had: no dw)   against   ..._bwd_dw_f32 (dw_out, domega_out)
  * kccot_weighted_sinkhorn_loss_bwd_f32                                         against   ..._bwd_dw_f32 (dw_real, dw_fake)
  * the adjoint of the weight estimator, kccot_conditional_weights_bwd_f32, alone.
configs[1] shape (64 x 64 frames, T = 30, J = 8), epsilon = 0.8, L = 100, option sinkhorn_shortcut = 0 so that every Sinkhorn
iteration runs.  The calls are interleaved (no-dw, dw, no-dw, dw, ...) so that clock drift hits both alike.  Prints ONE JSON
line.
usage: bench_weight_grad.py [--iters N] [--warmup N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from kccotgan_amd import _lib, gan_utils as G  # noqa: E402
from kccotgan_amd._lib import lib, check, ptr  # noqa: E402

EPS, LIT, LMIN, SC = 0.8, 100, 100, 1 / 15.0


def stats(t):
    t = sorted(t)
    pick = lambda q: t[min(len(t) - 1, int(q * len(t)))]
    return {"p10": pick(0.10), "p50": pick(0.50), "p90": pick(0.90), "mean": sum(t) / len(t)}


def interleaved_ms(fns, iters, warmup):
    """Event-timed eager calls of every function in turn, `iters` rounds after `warmup` rounds."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            evs[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in evs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.set_option("sinkhorn_shortcut", 0)
    B, H, T, W, C, J, Q = 64, 64, 30, 64, 1, 8, 64
    K = H * T * W * C
    gen = torch.Generator(device="cpu").manual_seed(1234)
    rnd = lambda *s: torch.rand(*s, generator=gen).cuda()
    real = rnd(B, K)
    fake = (real + 0.05 * torch.randn(real.shape, generator=gen).cuda()).clamp(0, 1)
    feats = [rnd(B, T, J) for _ in range(4)]                       # h_fake, h_real, m_real, m_fake
    ctx = real.view(B, H, T, W, C)[:, :, :10].contiguous()
    bw = 0.2 * (ctx[0].numel() ** 0.5)
    D = G.cost_xy(ctx, ctx, 1.0).contiguous()
    w = G.kernel_conditional_weights(ctx, bw)
    st = _lib.stream_of(real)
    f32 = lambda *s: torch.empty(*s, device="cuda")
    g1 = torch.ones(1, device="cuda")
    dfake, df = f32(B, K), [f32(B, T, J) for _ in range(4)]

    # ---- conditional loss: one forward, then the two backwards
    C3, uh, vh = f32(3, B, B), f32(Q, 3, LIT, B), f32(Q, 3, LIT, B)
    cost, nits, loss = f32(Q, 3), torch.empty(6 * Q, dtype=torch.int32, device="cuda"), f32(1)
    nb0 = lib.kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, Q)
    nb1 = lib.kccot_conditional_sinkhorn_loss_dw_workspace_bytes(B, K, Q)
    ws = torch.empty(max(nb0, nb1), dtype=torch.uint8, device="cuda")
    check(lib.kccot_conditional_sinkhorn_loss_fwd_f32(ptr(real), ptr(fake), B, K, SC, *map(ptr, feats), T, J, EPS, LIT, LMIN, 1e-2, 0,
                                                      ptr(w), None, Q, ptr(C3), ptr(uh), ptr(vh), ptr(cost), ptr(nits), ptr(loss),
                                                      ws.data_ptr(), nb0, st), "fwd")
    dw, dom = f32(Q, B), f32(Q)
    tail = (ptr(dfake), *map(ptr, df))
    head = (ptr(g1), ptr(real), ptr(fake), B, K, SC, *map(ptr, feats), T, J, EPS, LIT, ptr(w), None, Q, ptr(C3), ptr(uh), ptr(vh),
            ptr(nits))
    cond = {"conditional_bwd": lambda: check(lib.kccot_conditional_sinkhorn_loss_bwd_f32(*head, *tail, ws.data_ptr(), nb0, st), "bwd"),
            "conditional_bwd_dw": lambda: check(lib.kccot_conditional_sinkhorn_loss_bwd_dw_f32(
                *head, *tail, ptr(cost), ptr(dw), ptr(dom), ws.data_ptr(), nb1, st), "bwd_dw")}

    # ---- weighted loss
    C3w, uhw, vhw = f32(3, B, B), f32(3, LIT, B), f32(3, LIT, B)
    small, nitw, ticket = f32(4), torch.empty(6, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    mb0 = lib.kccot_weighted_sinkhorn_loss_workspace_bytes(B, K)
    mb1 = lib.kccot_weighted_sinkhorn_loss_dw_workspace_bytes(B, K)
    wsw = torch.empty(max(mb0, mb1), dtype=torch.uint8, device="cuda")
    wr, wf = w[0].contiguous(), w[1].contiguous()
    check(lib.kccot_weighted_sinkhorn_loss_fwd_f32(ptr(real), ptr(fake), B, K, SC, *map(ptr, feats), T, J, EPS, LIT, LMIN, 1e-2, 0,
                                                   ptr(wr), ptr(wf), ptr(C3w), ptr(uhw), ptr(vhw), ptr(small), ptr(nitw),
                                                   ptr(small[3:]), ptr(ticket), wsw.data_ptr(), mb0, st), "wfwd")
    dwr, dwf = f32(B), f32(B)
    headw = (ptr(g1), ptr(real), ptr(fake), B, K, SC, *map(ptr, feats), T, J, EPS, LIT, ptr(wr), ptr(wf), ptr(C3w), ptr(uhw),
             ptr(vhw), ptr(nitw))
    wtd = {"weighted_bwd": lambda: check(lib.kccot_weighted_sinkhorn_loss_bwd_f32(*headw, *tail, wsw.data_ptr(), mb0, st), "wbwd"),
           "weighted_bwd_dw": lambda: check(lib.kccot_weighted_sinkhorn_loss_bwd_dw_f32(*headw, *tail, ptr(dwr), ptr(dwf),
                                                                                         wsw.data_ptr(), mb1, st), "wbwd_dw")}
    dD, dbw = f32(Q, B), f32(Q)
    est = {"weights_bwd": lambda: check(lib.kccot_conditional_weights_bwd_f32(ptr(D), ptr(w), ptr(dw), Q, B, bw, ptr(dD), ptr(dbw), st),
                                        "weights_bwd")}

    t0 = time.time()
    rows = {}
    rows.update(interleaved_ms(cond, args.iters, args.warmup))
    rows.update(interleaved_ms(wtd, args.iters, args.warmup))
    rows.update(interleaved_ms(est, args.iters, args.warmup))
    torch.cuda.synchronize()
    res = {"shape": [B, H, T, W, C], "J": J, "Q": Q, "eps": EPS, "L": LIT, "iters": args.iters, "warmup": args.warmup,
           "sinkhorn_shortcut": 0, "launches": "eager", "unit": "ms", "rows": rows,
           "conditional_dw_over_plain_p50": rows["conditional_bwd_dw"]["p50"] / rows["conditional_bwd"]["p50"],
           "weighted_dw_over_plain_p50": rows["weighted_bwd_dw"]["p50"] / rows["weighted_bwd"]["p50"],
           "finite": bool(torch.isfinite(dw).all() and torch.isfinite(dom).all() and torch.isfinite(dwr).all()
                          and torch.isfinite(dD).all()),
           "wall_s": time.time() - t0}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
