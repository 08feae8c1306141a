"""Child process of tests/test_gpu_aniso_smoothing.py: gloo over a file store with world size 1.
KernelSmoothing(sharded=True).anisotropic_gaussian_convolution3D with two learnable sigmas must equal the unsharded call bit for
bit in out, x.grad and both sigma gradients (one rank: the all-reduces are identities and the local partials are the whole
gradients)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist


def main(store_path):
    from kccotgan_amd.data_utils import KernelSmoothing
    dist.init_process_group("gloo", store=dist.FileStore(store_path, 1), rank=0, world_size=1)
    try:
        dev = "cuda:0"
        gen = torch.Generator().manual_seed(7)
        x0 = torch.rand((2, 8, 9, 8, 2), generator=gen).to(dev)
        w = torch.randn((2, 8, 9, 8, 2), generator=gen).to(dev)
        done = 0
        for causal in (False, True):
            res = []
            for sharded in (False, True):
                ks = KernelSmoothing(4, 6, sharded=sharded)
                x = x0.clone().requires_grad_(True)
                sigma_t = torch.tensor(1.3, device=dev, requires_grad=True)
                sigma_s = torch.tensor(2.5, device=dev, requires_grad=True)
                out = ks.anisotropic_gaussian_convolution3D(x, sigma_t, sigma_s, causal=causal)
                (out * w).sum().backward()
                res.append((out.detach(), x.grad, sigma_t.grad.reshape(1), sigma_s.grad.reshape(1)))
            for a, b, what in zip(res[0], res[1], ("out", "x.grad", "sigma_t.grad", "sigma_s.grad")):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (causal, what, a.flatten()[:4], b.flatten()[:4])
            for v in res[0][2:]:
                assert float(v) != 0.0 and torch.isfinite(v).all()
            done += 1
        torch.cuda.synchronize()
        print("world1 ok %d" % done)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
