#!/usr/bin/env python3
"""RCCL check of the batch-sharded mixed Sinkhorn divergence on a one-GPU box: world size 1 over the nccl backend (two
ranks cannot share a card under RCCL), modelled on tools/nccl_bicausal_selftest.py.  At bench.py's configs[1] shape
(B = 64: the whole Cmix, the single-GPU loss call), the same shape with the row blocks forced (KCCOT_DIST_ROW_BLOCKS=1)
and at B = 128 on decimated frames (row blocks on the matrix pipe): the eager dist.sharded_mixed_sinkhorn_loss step --
whose four all_gather_into_tensor calls write the halves of the stacked R, F -- and the graph-captured
GraphedShardedMixedStep against the single-GPU compute_mixed_sinkhorn_loss.  Prints "nccl mixed selftest ok" on success.
Launch: a child process with MASTER_ADDR / MASTER_PORT / RANK=0 / WORLD_SIZE=1 / LOCAL_RANK=0 set
(tests/test_rccl_mixed_world1.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29519")
os.environ.setdefault("RANK", "0")
os.environ.setdefault("WORLD_SIZE", "1")
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)

from kccotgan_amd import dist as kd, gan_utils as G  # noqa: E402
from kccotgan_amd.graph import GraphedShardedMixedStep  # noqa: E402

FEATS = ("h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")
WRT = ("fake", "fake_p") + FEATS
SC = 1.0 / 15.0


def inputs(B, H, T, W, C, J, seed):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for r, f in (("real", "fake"), ("real_p", "fake_p")):
        t[r] = torch.rand(B, H, T, W, C, generator=g)
        t[f] = (t[r] + 0.05 * torch.randn(t[r].shape, generator=g)).clamp(0, 1)
    t.update({k: torch.rand(B, T, J, generator=g) for k in FEATS})
    return {k: v.to(dev) for k, v in t.items()}


def single_gpu(t):
    leaves = {k: t[k].clone().requires_grad_(True) for k in WRT}
    loss = G.compute_mixed_sinkhorn_loss(t["real"], leaves["fake"], t["real_p"], leaves["fake_p"], SC, 0.8, 100,
                                         *(leaves[k] for k in FEATS))
    return loss.detach(), torch.autograd.grad(loss, [leaves[k] for k in WRT])


def check_close(what, loss, grads, ref_loss, ref_grads, replicated):
    """replicated (the whole Cmix on every rank): the loss and the six feature gradients come from the single-GPU loss's
    own calls on the same operands and must be bit-identical; the two video gradients are the same product formed by the
    row form of the cost backward (two launches of a rank's rows instead of one over 2B), held to 1e-5 of max|grad|.
    Row blocks: two fp32 evaluations of different cost arithmetic.  W(x,x') and W(y,y') pair independent samples, so a
    cost matrix that differs by fp32 rounding moves the video gradient by up to the oracle's own fp32 / fp64 gap at this
    shape, 2.0e-4 of max|grad|: held to 2 x 4 x that gap, the rule of tests/test_dist_mixed.py."""
    if replicated:
        assert torch.equal(loss.reshape(()), ref_loss.reshape(())), (what, float(loss), float(ref_loss))
    else:
        assert abs(float(loss) - float(ref_loss)) <= 1e-4 * max(abs(float(ref_loss)), 1.0), (what, float(loss), float(ref_loss))
    worst = 0.0
    for k, g, r in zip(WRT, grads, ref_grads):
        if replicated and k in FEATS:
            assert torch.equal(g.reshape(r.shape), r), (what, k, "feature gradient differs from the single-GPU loss's")
            continue
        err = float((g.reshape(r.shape) - r).abs().max()) / max(float(r.abs().max()), 1e-30)
        assert err <= (1e-5 if replicated else 1.6e-3), (what, k, err)
        worst = max(worst, err)
    return worst


for name, shape, rows in (("configs[1]", (64, 64, 30, 64, 1, 8), False), ("configs[1] rows", (64, 64, 30, 64, 1, 8), True),
                          ("deci128", (128, 8, 10, 8, 4, 8), False)):
    if rows:
        os.environ["KCCOT_DIST_ROW_BLOCKS"] = "1"
    else:
        os.environ.pop("KCCOT_DIST_ROW_BLOCKS", None)
    t = inputs(*shape, seed=13)
    ref_loss, ref_grads = single_gpu(t)
    ref_C = G.last_info["compute_mixed_sinkhorn_loss_Cmix"].clone()
    shard = kd.shard_batch(t, 0, 1)
    loss, grads = kd.sharded_mixed_loss_step(shard, SC)
    torch.cuda.synchronize()
    replicated = name == "configs[1]"
    if replicated:                      # the whole Cmix: the single-GPU loss call on the gathered stacked videos
        assert torch.equal(kd.last_info["Cmix"], ref_C), "replicated Cmix differs from the single-GPU loss's"
    else:
        err = float((kd.last_info["Cmix"] - ref_C).abs().max()) / float(ref_C.abs().max())
        assert err <= 1e-5, (name, "Cmix", err)
    err = check_close(name + " eager", loss, grads, ref_loss, ref_grads, replicated)
    step = GraphedShardedMixedStep(shard, SC)
    assert step.replicated == replicated
    for _ in range(3):
        gl, gg = step()
    torch.cuda.synchronize()
    assert torch.equal(gl.reshape(()), loss.detach().reshape(())), (name, float(gl), float(loss))
    assert all(torch.equal(gg[k], g) for k, g in zip(WRT, grads)), (name, "graphed gradients")
    gl2, _ = step.step(fake_p=shard["fake_p"].detach() * 0.5)
    torch.cuda.synchronize()
    assert not torch.equal(gl2.reshape(()), loss.detach().reshape(())), (name, "replay ignores new inputs")
    print("%s: loss %.7g (single GPU %.7g), video gradients within %.2e, graphed step bit-identical"
          % (name, float(loss), float(ref_loss), err))
    del step
G.raise_if_solver_aborted(("compute_mixed_sinkhorn_loss",))
print("nccl mixed selftest ok: backend=%s" % dist.get_backend())
dist.destroy_process_group()
