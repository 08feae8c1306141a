#!/usr/bin/env python3
"""Loss + gradients of one of the Sinkhorn losses on seeded inputs, saved as .npy (bit-level A/B of two library builds or
two trees: run once per build with KCCOT_LIB_PATH, or once per tree, then tools/dump_loss_grads.py --compare a.npz b.npz).
  one      compute_sinkhorn_loss (default)
  bicausal compute_bicausal_sinkhorn_loss, same inputs
  mixed    compute_mixed_sinkhorn_loss: the same inputs as the first minibatch, a second one drawn after them"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--compare", nargs=2, metavar="NPZ")
ap.add_argument("--loss", choices=("one", "bicausal", "mixed"), default="one")
ap.add_argument("out", nargs="?")
ap.add_argument("shape", nargs="*", type=int)
args = ap.parse_args()
if args.compare:
    a, b = np.load(args.compare[0]), np.load(args.compare[1])
    bad = 0
    for k in a.files:
        same = a[k].tobytes() == b[k].tobytes()
        d = float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())
        print("%-10s %s  max|diff| %.3e" % (k, "bit-identical" if same else "DIFFERENT", d))
        bad += not same
    sys.exit(1 if bad else 0)
if not args.out or args.shape and len(args.shape) != 5:
    ap.error("give out.npz and optionally all of B H T W C")
import torch
from kccotgan_amd import gan_utils as G
B, H, T, W, C = args.shape or (64, 64, 30, 64, 1)
g = torch.Generator(device="cpu").manual_seed(1234)


def batch():
    real = torch.rand(B, H, T, W, C, generator=g).cuda()
    fake = (real + 0.05 * torch.randn(B, H, T, W, C, generator=g).cuda()).clamp(0, 1).requires_grad_(True)
    hs = [torch.rand(B, T - 1, 8, generator=g).cuda().requires_grad_(True) for _ in range(2)]    # h_fake, h_real
    ms = [torch.rand(B, T - 1, 8, generator=g).cuda().requires_grad_(True) for _ in range(2)]    # m_real, m_fake
    return real, fake, hs, ms


real, fake, hs, ms = batch()
if args.loss == "mixed":
    real_p, fake_p, hs_p, ms_p = batch()
    # h_fake, m_real, h_real', m_fake, h_fake', m_real'
    loss = G.compute_mixed_sinkhorn_loss(real, fake, real_p, fake_p, 1 / 15.0, 1.0, 100, hs[0], ms[0], hs_p[1], ms[1],
                                         hs_p[0], ms_p[0])
    wrt = {"dfake": fake, "dfake_p": fake_p, "dh_fake": hs[0], "dm_real": ms[0], "dh_real_p": hs_p[1], "dm_fake": ms[1],
           "dh_fake_p": hs_p[0], "dm_real_p": ms_p[0]}
else:
    fn = G.compute_sinkhorn_loss if args.loss == "one" else G.compute_bicausal_sinkhorn_loss
    loss = fn(real, fake, 1 / 15.0, 1.0, 100, hs[0], ms[0], hs[1], ms[1])
    wrt = {"dfake": fake, **{"dh%d" % i: h for i, h in enumerate(hs)}, **{"dm%d" % i: m for i, m in enumerate(ms)}}
loss.backward()
torch.cuda.synchronize()
np.savez(args.out, loss=loss.detach().cpu().numpy(), **{k: t.grad.cpu().numpy() for k, t in wrt.items()})
print("%s loss %.6f saved %s" % (args.loss, float(loss), args.out))
