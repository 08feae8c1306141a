#!/usr/bin/env python3
"""RCCL check of the batch-sharded RBF-kernel MMD on a one-GPU box: world size 1 over the nccl backend (two ranks cannot
share a card under RCCL), modelled on tools/nccl_mixed_selftest.py.  At bench.py's configs[1] video shape (B = 64: the
direct rows kernel) and at B = 128 and 256 on decimated frames (row blocks on the matrix pipe): dist.sharded_rbf_mmd2 --
whose all_gather_into_tensor calls write the preallocated [B,K] buffers, and whose kernel row blocks are all-gathered for
the backward -- forward and backward against the single-GPU mmd.rbf_mmd2 and the fp64 definition, with the bounds of
tests/test_gpu_dist_mmd.py; `gathered=` must give the same bits.  Prints "nccl mmd selftest ok" on success.
Launch: a child process with MASTER_ADDR / MASTER_PORT / RANK=0 / WORLD_SIZE=1 / LOCAL_RANK=0 set
(tests/test_gpu_dist_mmd.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29523")
os.environ.setdefault("RANK", "0")
os.environ.setdefault("WORLD_SIZE", "1")
dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
torch.cuda.set_device(dev)
dist.init_process_group("nccl", device_id=dev)

from kccotgan_amd import dist as kd, mmd  # noqa: E402


def fp64(x, y, gamma):
    xd, yd = x.double().cpu(), y.double().cpu().requires_grad_(True)
    kern = lambda a, b: torch.exp(-gamma * torch.cdist(a, b) ** 2)
    m = kern(xd, xd).mean() + kern(yd, yd).mean() - 2 * kern(xd, yd).mean()
    m.backward()
    return float(m.detach()), yd.grad


for name, shape, gamma in (("configs[1]", (64, 64, 30, 64, 1), None), ("deci128", (128, 8, 10, 8, 4), 0.0005),
                           ("deci256", (256, 8, 10, 8, 4), None)):
    g = torch.Generator().manual_seed(17)
    real = torch.rand(shape, generator=g)
    fake = (real + 0.2 * torch.randn(shape, generator=g)).clamp(0, 1)
    real, fake = real.to(dev), fake.to(dev)
    B = shape[0]
    gm = gamma if gamma is not None else 1.0 / real[0].numel()
    ref, gref = fp64(real.reshape(B, -1), fake.reshape(B, -1), gm)
    outs = []
    for fn in (lambda y: mmd.rbf_mmd2(real, y, gamma), lambda y: kd.sharded_rbf_mmd2(real, y, gamma),
               lambda y: kd.sharded_rbf_mmd2(real, y, gamma, gathered=(real, fake))):
        y = fake.clone().requires_grad_(True)
        m = fn(y)
        m.backward()
        torch.cuda.synchronize()
        outs.append((float(m.detach()), y.grad.reshape(B, -1).double().cpu()))
    (m1, g1), (ms, gs), (mg, gg) = outs
    assert ms == mg and torch.equal(gs, gg), (name, "gathered= changes the result")
    gmax = float(gref.abs().max())
    single_v, single_g = abs(m1 - ref), float((g1 - gref).abs().max()) / gmax
    sharded_v, sharded_g = abs(ms - ref), float((gs - gref).abs().max()) / gmax
    bound_v, bound_g = max(1e-5 * max(abs(ref), 1e-3), 1.25 * single_v), max(2e-5, 1.25 * single_g)
    print("%s: mmd^2 sharded %.9g, single GPU %.9g, fp64 %.9g; from fp64: %.2e / %.2e (value), %.2e / %.2e of max|grad|"
          % (name, ms, m1, ref, sharded_v, single_v, sharded_g, single_g))
    assert sharded_v <= bound_v and abs(ms - m1) <= 2.0 * bound_v, (name, ms, m1, ref)
    assert sharded_g <= bound_g, (name, sharded_g, single_g)
print("nccl mmd selftest ok: backend=%s" % dist.get_backend())
dist.destroy_process_group()
