"""Worker + test-only ops for the batch-sharded mixed Sinkhorn divergence (spawned by tests/test_dist_mixed.py).

argv: rank world port shape seed regime device mode out_pattern;  mode = "oracle" (CPU, MixedOracleOps) or "hip" (the HIP
library, plus the graph-captured step).  KCCOT_DIST_ROW_BLOCKS=1 in the environment forces the row-block regime."""
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
import mixed_cases  # noqa: E402
from oracle import gan_utils_torch as ot  # noqa: E402

WRT = ("fake", "fake_p", "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")


def batch(shape, seed, regime, world):
    """mixed_cases.gen_inputs, trimmed to the largest batch `world` divides (tiny's B = 5 -> 4 at two or four ranks).
    shape "name@N": the first N samples of `name` (a ragged batch); regime "near+zero": the four videos all zero."""
    name, _, n = shape.partition("@")
    base, _, zero = regime.partition("+")
    inp = mixed_cases.gen_inputs(name, seed, base)
    B = int(n) if n else inp["real"].shape[0]
    B = B // world * world
    out = {k: v[:B].copy() for k, v in inp.items()}
    if zero:
        for k in ("real", "fake", "real_p", "fake_p"):
            out[k][:] = 0.0
    return out


def single_gpu(inp):
    """compute_mixed_sinkhorn_loss of the whole batch on one GPU: loss, gradients (WRT order), Cmix, iteration counts."""
    from kccotgan_amd import gan_utils as G
    t = {k: torch.from_numpy(v).to("cuda:0") for k, v in inp.items()}
    for k in WRT:
        t[k].requires_grad_(True)
    loss = G.compute_mixed_sinkhorn_loss(*(t[k] for k in ("real", "fake", "real_p", "fake_p")), cases.SC, 0.8, 100,
                                         *(t[k] for k in mixed_cases.KEYS[4:]))
    tag = "compute_mixed_sinkhorn_loss"
    Cmix, nits = G.last_info[tag + "_Cmix"].cpu().numpy().copy(), G.last_info[tag].cpu().numpy().copy()
    grads = torch.autograd.grad(loss, [t[k] for k in WRT])
    out = {"ref_loss": np.array(float(loss)), "ref_Cmix": Cmix, "ref_nits": nits}
    out.update({"ref_d" + k: g.cpu().double().numpy() for k, g in zip(WRT, grads)})
    return out


def _d(a, b, sc):
    return ot.cost_xy(a.unsqueeze(1), b.unsqueeze(1), sc)


class MixedOracleOps:
    """CPU stand-in for the mixed operations of kccotgan_amd.dist.HipOps (dist.MIXED_OPS), built on the torch oracle in
    the inputs' dtype (fp64 in the tests) with autograd for the backward.  TEST ONLY: lets the gloo tests exercise the
    gathers, the stacked row-block indexing, the block map and the gradient rows of both regimes without a GPU."""

    @staticmethod
    def replicate_costs(B, K):
        # the rule of HipOps.replicate_costs, with the same KCCOT_DIST_ROW_BLOCKS switch
        return B <= 64 and K % 4 == 0 and K >= 256 and os.environ.get("KCCOT_DIST_ROW_BLOCKS") != "1"

    @staticmethod
    def mixed_loss_full(R, F, feats, sc, eps, L, keep):
        B = R.shape[0] // 2
        x, xp, y, yp = R[:B], R[B:], F[:B], F[B:]
        hf, mr, hrp, mf, hfp, mrp = feats
        Cmix = torch.stack([_d(x, y, sc) + ot.causal_term(hf, mr, sc), _d(xp, yp, sc) + ot.causal_term(hfp, mrp, sc),
                            _d(x, xp, sc) + ot.causal_term(hrp, mr, sc), _d(y, yp, sc) + ot.causal_term(hfp, mf, sc)])
        loss, st = MixedOracleOps.mixed_loss_given(Cmix, eps, L, keep)
        return loss, Cmix, st

    @staticmethod
    def mixed_cost_rows(R, F, sc, row_begin, row_count, norms=None):
        rows = slice(row_begin, row_begin + row_count)
        return torch.stack([_d(R[rows], F, sc), _d(R[rows], R, sc), _d(F[rows], F, sc)])

    @staticmethod
    def causal_add(C, h_rows, M, sc):
        return C + ot.causal_term(h_rows, M, sc)

    @staticmethod
    def mixed_loss_given(Cmix, eps, L, keep):
        with torch.enable_grad():
            leaf = Cmix.detach().clone().requires_grad_(True)
            c = [ot.sinkhorn_from_cost(leaf[p], eps, L)[0] for p in range(4)]
            loss = ((c[0] + c[1]) - c[2]) - c[3]
        return loss.detach(), (leaf, loss)

    @staticmethod
    def mixed_dcmix(st, g):
        leaf, loss = st
        return torch.autograd.grad(loss, leaf, g.to(loss.dtype))[0]

    @staticmethod
    def mixed_dfake_rows(dCmix, R, F, sc, row_begin, row_count):
        B = R.shape[0] // 2
        with torch.enable_grad():
            Fv = F.detach().clone().requires_grad_(True)
            C = torch.stack([_d(R[:B], Fv[:B], sc), _d(R[B:], Fv[B:], sc), _d(Fv[:B], Fv[B:], sc)])
            dF = torch.autograd.grad(C, Fv, torch.stack([dCmix[0], dCmix[1], dCmix[3]]))[0]
        return dF[row_begin:row_begin + row_count], dF[B + row_begin:B + row_begin + row_count]

    @staticmethod
    def mixed_feature_grads(dCmix, g, st, R, F, feats, sc, row_begin, row_count, whole=False):
        with torch.enable_grad():
            v = [t.detach().clone().requires_grad_(True) for t in feats]
            hf, mr, hrp, mf, hfp, mrp = v
            C = torch.stack([ot.causal_term(hf, mr, sc), ot.causal_term(hfp, mrp, sc), ot.causal_term(hrp, mr, sc),
                             ot.causal_term(hfp, mf, sc)])
            grads = torch.autograd.grad(C, v, dCmix)
        return tuple(t[row_begin:row_begin + row_count].contiguous() for t in grads)


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
    if use_hip:
        loss, grads = kd.sharded_mixed_loss_step(shard, cases.SC)
    else:
        loss = kd.sharded_mixed_sinkhorn_loss(shard["real"].detach(), shard["fake"], shard["real_p"].detach(), shard["fake_p"],
                                              cases.SC, *(shard[k] for k in mixed_cases.KEYS[4:]), ops=MixedOracleOps)
        grads = torch.autograd.grad(loss, [shard[k] for k in WRT])
    res = {"loss": np.array(float(loss))}
    for k, g in zip(WRT, grads):
        res["d" + k] = g.detach().cpu().double().numpy()
    if use_hip:
        tag = "compute_mixed_sinkhorn_loss"
        res["Cmix"] = kd.last_info["Cmix"].cpu().numpy()
        res["nits"] = G.last_info[tag].cpu().numpy()
        res["nits_executed"] = G.last_info[tag + "_executed"].cpu().numpy()
        res["nits_is_sharded"] = np.array(G.last_info[tag] is kd.last_info["nits"])
        G.raise_if_solver_aborted((tag,))
        # the graph-captured form of the same step: bit-identical, and it sees new inputs
        from kccotgan_amd.graph import GraphedShardedMixedStep
        step = GraphedShardedMixedStep(shard, cases.SC, L=100)
        for _ in range(2):
            gl, gg = step()
        res["graphed_loss_equal"] = np.array(bool(torch.equal(gl.reshape(()), loss.detach().reshape(()))))
        res["graphed_grads_equal"] = np.array(all(bool(torch.equal(gg[k], g)) for k, g in zip(WRT, grads)))
        res["graphed_replicated"] = np.array(step.replicated)
        gl2, _ = step.step(fake=shard["fake"].detach() * 0.5)
        res["graphed_sees_new_inputs"] = np.array(not bool(torch.equal(gl2, loss.detach().reshape(()))))
        if rank == 0:                    # the single-GPU loss on the whole batch, in this process: no extra GPU process
            res.update(single_gpu(inp))
    np.savez(out_path % rank, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    a = sys.argv
    run(int(a[1]), int(a[2]), int(a[3]), a[4], int(a[5]), a[6], a[7], a[8] == "hip", a[9])
