#!/usr/bin/env python3
"""RCCL check of the batch-sharded bi-causal loss on a one-GPU box: world size 1 over the nccl backend (two ranks cannot
share a card under RCCL), modelled on tools/nccl_selftest.py.  At bench.py's configs[1] shape (B = 64: replicated cost
assembly) and at B = 128 on decimated frames (row blocks), the eager dist.sharded_bicausal_sinkhorn_loss step, the
graph-captured GraphedShardedStep(bi_causal=True) and the contraction-sharded protocol (eager and GraphedKSplitStep)
against the single-GPU compute_bicausal_sinkhorn_loss.  Prints "nccl bicausal selftest ok" on success.
Launch: a child process with MASTER_ADDR / MASTER_PORT / RANK=0 / WORLD_SIZE=1 / LOCAL_RANK=0 set (tests/test_rccl_bicausal_world1.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29513")
os.environ.setdefault("RANK", "0")
os.environ.setdefault("WORLD_SIZE", "1")
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)

from kccotgan_amd import dist as kd, gan_utils as G  # noqa: E402
from kccotgan_amd.graph import GraphedKSplitStep, GraphedShardedStep  # noqa: E402

NAMES = ("fake", "h_fake", "h_real", "m_real", "m_fake")
SC = 1.0 / 15.0


def inputs(B, H, T, W, C, J, seed):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(B, H, T, W, C, generator=g)
    fake = (real + 0.05 * torch.randn(real.shape, generator=g)).clamp(0, 1)
    t = {"real": real, "fake": fake}
    t.update({k: torch.rand(B, T, J, generator=g) for k in ("h_fake", "h_real", "m_real", "m_fake")})
    return {k: v.to(dev) for k, v in t.items()}


def single_gpu(t):
    leaves = {k: t[k].clone().requires_grad_(True) for k in NAMES}
    loss = G.compute_bicausal_sinkhorn_loss(t["real"], leaves["fake"], SC, 0.8, 100, leaves["h_fake"], leaves["m_real"],
                                            leaves["h_real"], leaves["m_fake"])
    return loss.detach(), torch.autograd.grad(loss, [leaves[k] for k in NAMES])


def check_close(what, loss, grads, ref_loss, ref_grads, rtol):
    assert abs(float(loss) - float(ref_loss)) <= rtol * abs(float(ref_loss)), (what, float(loss), float(ref_loss))
    for k, g, r in zip(NAMES, grads, ref_grads):
        err = float((g.reshape(r.shape) - r).abs().max()) / max(float(r.abs().max()), 1e-30)
        assert err <= 1e-4, (what, k, err)


for name, shape in (("configs[1]", (64, 64, 30, 64, 1, 8)), ("deci128", (128, 8, 10, 8, 4, 8))):
    t = inputs(*shape, seed=11)
    ref_loss, ref_grads = single_gpu(t)
    ref_C3 = G.last_info["compute_bicausal_sinkhorn_loss_C3"].clone()
    shard = kd.shard_batch(t, 0, 1)
    for protocol, cls in (("gather", GraphedShardedStep), ("ksplit", GraphedKSplitStep)):
        loss, grads = kd.sharded_loss_step(shard, SC, protocol=protocol, bi_causal=True)
        torch.cuda.synchronize()
        if protocol == "gather" and name == "configs[1]":     # replicated assembly: the single-GPU loss's cost kernels
            assert torch.equal(kd.last_info["C3"], ref_C3), "replicated C3 differs from the single-GPU loss's"
        check_close("%s %s eager" % (name, protocol), loss, grads, ref_loss, ref_grads, 5e-6)
        step = cls(shard, SC, bi_causal=True)
        for _ in range(3):
            gl, gg = step()
        torch.cuda.synchronize()
        assert torch.equal(gl.reshape(()), loss.detach().reshape(())), (name, protocol, float(gl), float(loss))
        assert all(torch.equal(gg[k], g) for k, g in zip(NAMES, grads)), (name, protocol, "graphed gradients")
        gl2, _ = step(fake=shard["fake"].detach() * 0.5)
        torch.cuda.synchronize()
        assert not torch.equal(gl2.reshape(()), loss.detach().reshape(())), (name, protocol, "replay ignores new inputs")
        print("%s %s: loss %.7g (single GPU %.7g), graphed step bit-identical" % (name, protocol, float(loss), float(ref_loss)))
G.raise_if_solver_aborted(("compute_bicausal_sinkhorn_loss",))
print("nccl bicausal selftest ok: backend=%s" % dist.get_backend())
dist.destroy_process_group()
