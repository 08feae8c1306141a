"""Worker + test-only ops for the batch-sharded bi-causal loss (spawned by tests/test_dist_bicausal.py).

argv: rank world port shape seed regime device mode out_pattern;  mode = "oracle" (CPU, the ops below), "hip" (the HIP
library, plus the graph-captured steps) or "train" (one data-parallel KCCOTTrainer(bi_causal=True) iteration)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
from dist_worker import OracleOps  # noqa: E402
from oracle import gan_utils_torch as ot  # noqa: E402

NAMES = ("fake", "h_fake", "h_real", "m_real", "m_fake")


def batch(shape, seed, regime, world):
    """cases.gen_inputs, trimmed to the largest batch `world` divides (tiny's B = 5 -> 4: a shard per rank)."""
    inp = cases.gen_inputs(shape, seed, regime)
    B = inp["real"].shape[0] // world * world
    return {k: v[:B] for k, v in inp.items()}


class BicausalOracleOps(OracleOps):
    """The torch oracle's one-batch ops (tests/dist_worker.py) extended with the two bi-causal operations of
    kccotgan_amd.dist.HipOps: the second causal term of each matrix, and the feature gradients through the bi-causal cost
    (ot.bi_causal_modified_cost).  TEST ONLY."""

    @staticmethod
    def bicausal_term(C3, h_fake, h_real, m_real, m_fake, sc):
        return C3 + torch.stack([ot.causal_term(h_real, m_fake, sc), ot.causal_term(h_real, m_real, sc),
                                 ot.causal_term(h_fake, m_fake, sc)])

    @staticmethod
    def bicausal_feature_grads(dC3, real, fake, h_fake, h_real, m_real, m_fake, sc, row_begin, row_count, whole=False):
        with torch.enable_grad():
            v = [t.detach().clone().requires_grad_(True) for t in (h_fake, h_real, m_real, m_fake)]
            hf, hr, mr, mf = v
            x, y = real.unsqueeze(1), fake.unsqueeze(1)
            C3 = torch.stack([ot.bi_causal_modified_cost(x, y, hf, mr, hr, mf, sc),
                              ot.bi_causal_modified_cost(x, x, hr, mr, hr, mr, sc),
                              ot.bi_causal_modified_cost(y, y, hf, mf, hf, mf, sc)])
            grads = torch.autograd.grad(C3, v, dC3)
        return tuple(g[row_begin:row_begin + row_count].contiguous() for g in grads)


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def run(rank, world, port, shape, seed, regime, device, use_hip, out_path):
    _init(rank, world, port)
    from kccotgan_amd import dist as kd
    from kccotgan_amd import gan_utils as G
    inp = batch(shape, seed, regime, world)
    dtype = torch.float32 if use_hip else torch.float64
    t = {k: torch.from_numpy(v).to(dtype).to(device) for k, v in inp.items()}
    shard = kd.shard_batch(t, rank, world)
    loss = kd.sharded_bicausal_sinkhorn_loss(shard["real"], shard["fake"], cases.SC, shard["h_fake"], shard["m_real"],
                                             shard["h_real"], shard["m_fake"], ops=None if use_hip else BicausalOracleOps)
    grads = torch.autograd.grad(loss, [shard[k] for k in NAMES])
    res = {"loss": np.array(float(loss))}
    for k, g in zip(NAMES, grads):
        res["d" + k] = g.detach().cpu().double().numpy()
    if use_hip:
        tag = "compute_bicausal_sinkhorn_loss"
        res["C3"] = kd.last_info["C3"].cpu().numpy()
        res["nits"] = G.last_info[tag].cpu().numpy()
        res["nits_executed"] = G.last_info[tag + "_executed"].cpu().numpy()
        res["nits_is_sharded"] = np.array(G.last_info[tag] is kd.last_info["nits"])
        # the graph-captured form of the same step: bit-identical, and it sees new inputs
        from kccotgan_amd.graph import GraphedKSplitStep, GraphedShardedStep
        cls = GraphedKSplitStep if os.environ.get("KCCOT_DIST_PROTOCOL") == "ksplit" else GraphedShardedStep
        step = cls(shard, cases.SC, L=100, bi_causal=True)
        for _ in range(2):
            gl, gg = step()
        res["graphed_loss_equal"] = np.array(bool(torch.equal(gl.reshape(()), loss.detach().reshape(()))))
        res["graphed_grads_equal"] = np.array(all(bool(torch.equal(gg[k], g)) for k, g in zip(NAMES, grads)))
        gl2, _ = step(fake=shard["fake"].detach() * 0.5)
        res["graphed_sees_new_inputs"] = np.array(not bool(torch.equal(gl2, loss.detach().reshape(()))))
    np.savez(out_path % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


def run_train(rank, world, port, seed, device, out_path):
    """One data-parallel iteration (disc + gen step) of KCCOTTrainer(bi_causal=True) on `world` ranks."""
    _init(rank, world, port)
    from kccotgan_amd import dist as kd
    from kccotgan_amd import gan, gan_utils as G
    from kccotgan_amd.kernel_train import KCCOTTrainer
    gan._NATIVE = {"convlstm", "deconv", "dconv"}            # conservative convolution mode, as tests/dist_worker.py
    Bl, H, W, C, T, iT = 2, 64, 64, 1, 6, 2
    tr = KCCOTTrainer(Bl, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="1d", warmup=10,
                      device=device, seed=seed + rank, bi_causal=True)
    x = torch.from_numpy(np.random.default_rng(7).random((Bl * world, H, T, W, C), dtype=np.float32))[rank * Bl:(rank + 1) * Bl]
    p0 = torch.cat([p.detach().reshape(-1) for p in tr.g_params + tr.d_params]).cpu().numpy()
    G.last_info.pop("compute_bicausal_sinkhorn_loss", None)
    kd.last_info.pop("C3", None)
    pm, loss = tr.train_iteration(x.to(device), 4.0)
    p1 = torch.cat([p.detach().reshape(-1) for p in tr.g_params + tr.d_params]).cpu().numpy()
    ran = "compute_bicausal_sinkhorn_loss" in G.last_info and "C3" in kd.last_info
    G.raise_if_solver_aborted(("compute_bicausal_sinkhorn_loss",))
    np.savez(out_path % rank, p0=p0, p1=p1, pm=np.array(float(pm)), loss=np.array(float(loss)), ran_sharded=np.array(ran),
             B=np.array(int(kd.last_info["C3"].shape[1]) if ran else 0))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    if a[8] == "train":
        run_train(int(a[1]), int(a[2]), int(a[3]), int(a[5]), a[7], a[9])
    else:
        run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), a[6], a[7], a[8] == "hip", a[9])
