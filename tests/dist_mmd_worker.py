"""Worker + test-only ops for the batch-sharded RBF-kernel MMD (spawned by tests/test_dist_mmd.py and
tests/test_gpu_dist_mmd.py).

argv: rank world port case device mode out_pattern;  mode = "oracle" (CPU, MMDOracleOps, fp64) or "hip" (the HIP library).
case = "B,K,seed,regime,gamma": regime near / far / same (fake == real), gamma a float or "none" (1 / K)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def batch(case):
    """(real, fake) [B,K] fp32 and gamma: real uniform in [0,1); near: fake = clip(real + 0.2 N(0,1)) (the inputs of
    tests/test_gpu_parity.py's rbf_mmd tests); far: an independent uniform batch; same: fake == real."""
    B, K, seed, regime, gamma = case.split(",")
    if not B.isdigit():                  # "small,-,seed,regime,gamma": the videos of cases.gen_inputs(name, seed, regime)
        import cases
        inp = cases.gen_inputs(B, int(seed), regime)
        n = inp["real"].shape[0]
        return inp["real"].reshape(n, -1), inp["fake"].reshape(n, -1), (None if gamma == "none" else float(gamma))
    B, K = int(B), int(K)
    rng = np.random.default_rng(int(seed))
    x = rng.random((B, K), dtype=np.float32)
    if regime == "near":
        y = np.clip(x + 0.2 * rng.standard_normal((B, K), dtype=np.float32), 0, 1).astype(np.float32)
    elif regime == "far":
        y = rng.random((B, K), dtype=np.float32)
    elif regime == "same":
        y = x.copy()
    else:
        raise ValueError(regime)
    return x, y, (None if gamma == "none" else float(gamma))


def definition(x, y, gamma, dtype=torch.float64, weight=3.0):
    """mmd^2 = mean(Kxx) + mean(Kyy) - 2 mean(Kxy), K = exp(-gamma |a-b|^2), and d (weight mmd^2) / d y by autograd."""
    xd = torch.from_numpy(x).to(dtype)
    yd = torch.from_numpy(y).to(dtype).requires_grad_(True)
    gm = gamma if gamma is not None else 1.0 / x.shape[1]
    kern = lambda a, b: torch.exp(-gm * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    m = kern(xd, xd).mean() + kern(yd, yd).mean() - 2 * kern(xd, yd).mean()
    (weight * m).backward()
    return float(m.detach()), yd.grad.numpy()


def definition_value(x, y, gamma):
    """The value of the same definition on the same inputs, evaluated so that its OWN rounding stays well below 1e-12 of
    the result: mmd^2 is a difference of means of size ~1 (2.8e-4 on the near batch), so one fp64 rounding of a mean
    (1.1e-16) is already 4e-13 of it, and torch's fp64 evaluation above sits 1.3e-12 from the exact value there.
    numpy's extended precision where it has one (x86: 64-bit mantissa), else fp64 entries with exactly rounded sums."""
    import math
    ext = np.longdouble if np.finfo(np.longdouble).eps < 1e-18 else np.float64
    gm = ext(gamma if gamma is not None else 1.0 / x.shape[1])          # the fp64 gamma the code is given
    X, Y = x.astype(ext), y.astype(ext)
    kern = lambda a, b: np.exp(-gm * ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1))
    n = ext(x.shape[0]) ** 2
    if ext is np.longdouble:
        s = [kern(X, X).sum(), kern(Y, Y).sum(), kern(X, Y).sum()]
        return float((s[0] + s[1] - 2 * s[2]) / n)
    kxx, kyy, kxy = kern(X, X).ravel(), kern(Y, Y).ravel(), kern(X, Y).ravel()
    return math.fsum(list(kxx) + list(kyy) + list(-2.0 * kxy)) / float(n)


def _d2(a, b):
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)


class MMDOracleOps:
    """CPU stand-in for the MMD operations of kccotgan_amd.dist.HipOps (dist.MMD_OPS) in the inputs' dtype (fp64 in the
    tests).  TEST ONLY: lets the gloo tests exercise the gathers, the row-block indexing, the all-reduce of the three sums
    and the gradient rows without a GPU."""

    @staticmethod
    def mmd_cost_rows(real, fake, row_begin, row_count, norms=None):
        rows = slice(row_begin, row_begin + row_count)
        return torch.stack([_d2(real[rows], fake), _d2(real[rows], real), _d2(fake[rows], fake)])

    @staticmethod
    def rbf_sum_rows(blk, gamma):
        K = torch.exp(-gamma * blk)
        return K, K.sum(dim=(1, 2))

    @staticmethod
    def rbf_mmd_grad(K3, gamma, g):
        coef = torch.tensor([-2.0, 1.0, 1.0], dtype=K3.dtype).reshape(3, 1, 1)
        return g.to(K3.dtype) * coef * (-gamma) * K3 / float(K3.shape[1] * K3.shape[2])

    @staticmethod
    def dfake_rows(gD3, real, fake, sc, row_begin, row_count):
        with torch.enable_grad():
            f = fake.detach().clone().requires_grad_(True)
            D3 = sc * torch.stack([_d2(real, f), _d2(real, real), _d2(f, f)])
            df = torch.autograd.grad(D3, f, gD3)[0]
        return df[row_begin:row_begin + row_count].contiguous()


def run(rank, world, port, case, device, use_hip, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from kccotgan_amd import dist as kd
    x, y, gamma = batch(case)
    dtype = torch.float32 if use_hip else torch.float64
    B = x.shape[0]
    Bl = B // world
    X, Y = torch.from_numpy(x).to(dtype).to(device), torch.from_numpy(y).to(dtype).to(device)
    xl = X[rank * Bl:(rank + 1) * Bl].contiguous()
    yl = Y[rank * Bl:(rank + 1) * Bl].clone().requires_grad_(True)
    ops = None if use_hip else MMDOracleOps
    m = kd.sharded_rbf_mmd2(xl, yl, gamma, ops=ops)
    (3.0 * m).backward()
    res = {"mmd": np.array(float(m.detach().double())), "dtype": np.array(str(m.dtype)), "dfake": yl.grad.detach().cpu().double().numpy()}
    # the videos already gathered: the same bits, value and gradient; and a forward-only evaluation
    yl2 = yl.detach().clone().requires_grad_(True)
    m2 = kd.sharded_rbf_mmd2(xl, yl2, gamma, ops=ops, gathered=(X, Y))
    (3.0 * m2).backward()
    res["gathered_equal"] = np.array(bool(torch.equal(m2.detach(), m.detach())) and bool(torch.equal(yl2.grad, yl.grad)))
    with torch.no_grad():
        res["nograd_equal"] = np.array(bool(torch.equal(kd.sharded_rbf_mmd2(xl, yl.detach(), gamma, ops=ops), m.detach())))
    if use_hip and rank == 0:            # the single-GPU call on the whole batch, in this process: no extra GPU process
        from kccotgan_amd import mmd
        Yr = Y.clone().requires_grad_(True)
        ms = mmd.rbf_mmd2(X, Yr, gamma)
        (3.0 * ms).backward()
        res["ref_mmd"] = np.array(float(ms.detach().double()))
        res["ref_dfake"] = Yr.grad.cpu().double().numpy()
    np.savez(out_path % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], a[5], a[6] == "hip", a[7])
