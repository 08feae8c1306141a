"""GPU tier of the batch-sharded RBF-kernel MMD (kccotgan_amd.dist.sharded_rbf_mmd2): two ranks over gloo sharing cuda:0
(four at B = 256) with the HIP library, arranged as the sharded mixed tests are (tests/test_dist_mixed.py): the workers
(tests/dist_mmd_worker.py, each under its own time limit) are the only GPU processes started, rank 0 evaluates the
single-GPU mmd.rbf_mmd2 itself.  Bounds: the ones tests/test_gpu_parity.py applies to the single-GPU call
(test_rbf_mmd_matches_sklearn_definition: 1e-5 of max(|mmd^2|, 1e-3); test_rbf_mmd_gradient_wrt_fake: 2e-5 of max|grad|; at
fake == real |mmd^2| <= 1e-6) -- or, where the single-GPU call on the same input is itself farther from fp64, at most 1.25 x
its distance (the rule of DESIGN.md section 10.1).  Then RCCL at world size 1 in a child process, the call without a
process group, and KCCOTTrainer.mmd."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dist_mmd_worker as w
from test_dist_mmd import free_port, launch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case,world,gram", [
    ("64,1920,0,near,none", 2, False),        # Bl = 32, B = 64: the direct rows kernel
    ("128,512,1,near,0.01", 2, True),         # Bl = 64, B = 128: the matrix pipe, an explicit gamma
    ("128,2560,2,far,none", 4, True),         # Bl = 32, B = 128: the matrix pipe, independent batches
    ("256,2560,3,near,none", 4, True),        # Bl = 64, B = 256 (four worker processes on the GPU)
])
def test_sharded_mmd_hip(case, world, gram, tmp_path):
    from kccotgan_amd import _lib
    x, y, gamma = w.batch(case)
    B, K = x.shape
    Bl = B // world
    assert bool(_lib.lib.kccot_pairwise_cost3_rows_gram_supported(Bl, B, K)) == gram
    res = launch(world, case, "cuda:0", "hip", tmp_path)
    ref, gref = w.definition(x, y, gamma)
    gmax = np.abs(gref).max()
    ref_mmd, ref_g = float(res[0]["ref_mmd"]), res[0]["ref_dfake"]
    single_v, single_g = abs(ref_mmd - ref), float(np.abs(ref_g - gref).max()) / gmax
    tol_v = 1e-5 * max(abs(ref), 1e-3)
    bound_v, bound_g = max(tol_v, 1.25 * single_v), max(2e-5, 1.25 * single_g)
    for r, out in enumerate(res):
        assert str(out["dtype"]) == "torch.float32"
        assert float(out["mmd"]) == float(res[0]["mmd"])                    # identical bits on all ranks
        assert bool(out["gathered_equal"]) and bool(out["nograd_equal"])
        sharded_v = abs(float(out["mmd"]) - ref)
        rows = gref[r * Bl:(r + 1) * Bl]
        sharded_g = float(np.abs(out["dfake"] - rows).max()) / gmax
        print("%s rank %d: mmd^2 %.9g (fp64 %.9g): sharded %.2e, single GPU %.2e from fp64 (tol %.2e); gradient: sharded "
              "%.2e, single GPU %.2e of max|grad| (tol 2e-5)" % (case, r, float(out["mmd"]), ref, sharded_v, single_v, tol_v,
                                                                 sharded_g, single_g))
        assert sharded_v <= bound_v, "mmd^2 vs fp64: %.3e > %.3e (single GPU %.3e)" % (sharded_v, bound_v, single_v)
        assert abs(float(out["mmd"]) - ref_mmd) <= 2.0 * bound_v                    # HIP against HIP
        assert sharded_g <= bound_g, "gradient vs fp64: %.3e > %.3e (single GPU %.3e)" % (sharded_g, bound_g, single_g)
        np.testing.assert_allclose(out["dfake"], ref_g[r * Bl:(r + 1) * Bl], rtol=0, atol=2.0 * bound_g * gmax)


@pytest.mark.parametrize("case,world", [("64,1920,4,same,none", 2), ("128,512,5,same,none", 2)])
def test_sharded_mmd_of_identical_batches_is_zero(case, world, tmp_path):
    """fake == real (direct rows at B = 64, the matrix pipe at B = 128): |mmd^2| <= 1e-6, as tests/test_gpu_parity.py asks
    of the single-GPU call."""
    res = launch(world, case, "cuda:0", "hip", tmp_path)
    for out in res:
        print("%s: mmd^2 %.3e (single GPU %.3e)" % (case, float(out["mmd"]), float(res[0]["ref_mmd"])))
        assert abs(float(out["mmd"])) <= 1e-6 and float(out["mmd"]) == float(res[0]["mmd"])
        assert np.isfinite(out["dfake"]).all()


def test_rccl_sharded_mmd_at_world_size_1():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("KCCOT_DIST_ROWS", None)
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(ROOT, "tools", "nccl_mmd_selftest.py")],
                       env=env, capture_output=True, text=True, timeout=640)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "nccl mmd selftest ok: backend=nccl" in p.stdout, p.stdout[-2000:]


def test_without_a_process_group_it_is_the_single_gpu_call():
    import torch.distributed as dist
    from kccotgan_amd import dist as kd, mmd
    assert not dist.is_initialized()
    x, y, _ = w.batch("16,320,6,near,none")
    X = torch.from_numpy(x).cuda()
    for gamma in (None, 0.01):
        Y1, Y2 = (torch.from_numpy(y).cuda().requires_grad_(True) for _ in range(2))
        a, b = kd.sharded_rbf_mmd2(X, Y1, gamma), mmd.rbf_mmd2(X, Y2, gamma)
        assert torch.equal(a.detach(), b.detach())
        a.backward()
        b.backward()
        assert torch.equal(Y1.grad, Y2.grad)


def test_trainer_mmd_is_a_monitor(monkeypatch):
    from kccotgan_amd import gan
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2
    tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="1d", warmup=10,
                      device="cuda:0")
    x = torch.rand(B, H, T, W, C, device="cuda:0")
    nets = (tr.context_encoder, tr.decoder, tr.discriminator_h, tr.discriminator_m)
    snap = lambda: [t.detach().clone() for n in nets for t in list(n.parameters()) + list(n.buffers())]
    before = snap()
    its = (tr.gen_optimiser.iterations, tr.dischm_optimiser.iterations)
    for sigma in (None, 5.0):
        m = tr.mmd(x, sigma)
        assert m.dim() == 0 and not m.requires_grad and bool(torch.isfinite(m))
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    assert (tr.gen_optimiser.iterations, tr.dischm_optimiser.iterations) == its
