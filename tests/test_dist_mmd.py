"""The batch-sharded RBF-kernel MMD (kccotgan_amd.dist.sharded_rbf_mmd2), CPU tier: its signature, the protocol over gloo
at world sizes 2 and 4 with fp64 oracle operations (tests/dist_mmd_worker.py) against the fp64 whole-batch definition, the
refusals before any collective, and the new ABI flag KCCOT_COST_RBF_SUM's refusals on its arguments (no launch).  The GPU
tier is tests/test_gpu_dist_mmd.py and tests/test_gpu_rbf_flag_bounds.py."""
import inspect
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(world, case, device, mode, tmp_path, env=None, timeout=600):
    """One worker per rank, each under its own time limit; a rank that fails ends the run."""
    port = free_port()
    out = os.path.join(str(tmp_path), "rank%d.npz")
    procs = [subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, os.path.join(HERE, "dist_mmd_worker.py"),
                               str(r), str(world), str(port), case, device, mode, out], env=dict(os.environ, **(env or {})))
             for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=timeout + 30) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(out % r) for r in range(world)]


def test_public_signature():
    """Fails on the parent commit (AttributeError): the function is new."""
    from kccotgan_amd import dist as kd
    sig = inspect.signature(kd.sharded_rbf_mmd2)
    assert list(sig.parameters) == ["real_l", "fake_l", "gamma", "group", "ops", "gathered"]
    assert all(sig.parameters[k].default is None for k in ("gamma", "group", "ops", "gathered"))
    assert set(kd.MMD_OPS) <= set(dir(kd.HipOps))
    from kccotgan_amd.kernel_train import KCCOTTrainer
    assert list(inspect.signature(KCCOTTrainer.mmd).parameters) == ["self", "real_data", "sigma"]


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("case", ["small,-,0,near,none", "small,-,1,far,none", "small,-,0,near,0.05", "small,-,1,far,0.002"])
def test_sharded_mmd_equals_fp64_definition(world, case, tmp_path):
    """fp64 protocol against the whole-batch definition: the gathers, the row blocks, the all-reduce of the three sums and
    each rank's gradient rows.  The value's reference is the definition evaluated beyond fp64 (dist_mmd_worker.
    definition_value): at 1e-12 of a difference of means the plain fp64 evaluation is not accurate enough to be one --
    measured on small / seed 0 / near, default gamma: torch fp64 definition 1.3e-12 from the extended-precision value, the
    sharded fp64 protocol 3.5e-13 (both world sizes); the other three cases 4e-15 .. 2e-14.  Gradient: fp64 autograd."""
    import dist_mmd_worker as w
    res = launch(world, case, "cpu", "oracle", tmp_path)
    x, y, gamma = w.batch(case)
    ref64, gref = w.definition(x, y, gamma)
    ref = w.definition_value(x, y, gamma)
    assert abs(ref64 - ref) <= 1e-11 * abs(ref)                                 # the two evaluations describe one quantity
    Bl = x.shape[0] // world
    got = np.concatenate([out["dfake"] for out in res], axis=0)
    for out in res:
        assert str(out["dtype"]) == "torch.float64"
        assert abs(float(out["mmd"]) - ref) <= 1e-12 * abs(ref), (float(out["mmd"]), ref)
        assert float(out["mmd"]) == float(res[0]["mmd"])                    # identical bits on all ranks
        assert out["dfake"].shape == (Bl, x.shape[1])
        assert bool(out["gathered_equal"]) and bool(out["nograd_equal"])
    np.testing.assert_allclose(got, gref, rtol=0, atol=1e-10 * np.abs(gref).max())


def test_refusals_come_before_any_collective():
    """No process group exists here: every refusal must come before the first collective, with a message that names it."""
    from dist_mmd_worker import MMDOracleOps
    from dist_worker import OracleOps
    from kccotgan_amd import dist as kd
    x, y = torch.rand(4, 3, 5, dtype=torch.float64), torch.rand(4, 3, 5, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="mmd_cost_rows"):           # ops without the MMD operations
        kd.sharded_rbf_mmd2(x, y, ops=OracleOps)
    with pytest.raises(NotImplementedError, match="never differentiates w.r.t. real"):
        kd.sharded_rbf_mmd2(x.clone().requires_grad_(True), y, ops=MMDOracleOps)
    with pytest.raises(ValueError, match="same shape"):
        kd.sharded_rbf_mmd2(x, y[:-1], ops=MMDOracleOps)
    with pytest.raises(ValueError, match="same shape"):
        kd.sharded_rbf_mmd2(x, y[:, :, :-1], ops=MMDOracleOps)
    for g in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            kd.sharded_rbf_mmd2(x, y, gamma=g, ops=MMDOracleOps)
    with pytest.raises(ValueError, match="gathered"):
        kd.sharded_rbf_mmd2(x, y, ops=MMDOracleOps, gathered=(x, y[:, :, :-1]))
    assert set(kd.MMD_OPS) <= set(dir(MMDOracleOps))


def test_rbf_sum_flag_is_declared_and_refused_on_its_arguments():
    """KCCOT_COST_RBF_SUM = 512 (kccot_pairwise_cost_f32) in the header and the binding; with any other flag, without
    C_out / ws, with sc <= 0, a bad shape or a short workspace the call is rejected on its arguments (no launch: this runs
    without a GPU); kccot_pairwise_cost3_f32 and the loss entry points refuse it."""
    from kccotgan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "kccot.h")).read()
    assert re.search(r"#define KCCOT_COST_RBF_SUM 512u", hdr)
    assert _lib.COST_RBF_SUM == 512
    lib, one = _lib.lib, 16
    R = _lib.COST_RBF_SUM
    need = int(lib.kccot_pairwise_cost_workspace_bytes(8, 9, 1))
    assert need >= 8 * (1 + 2 * 1)                       # the sum and one partial per 4 x 64 tile

    def call(flags, Bx=8, By=9, sc=0.5, C=one, ws=one, wsb=None):
        nb = int(lib.kccot_pairwise_cost_workspace_bytes(Bx, By, 1)) if wsb is None else wsb
        return lib.kccot_pairwise_cost_f32(None, None, Bx, By, 0, sc, None, None, None, None, 0, 0, flags, C, ws, nb, None)

    for other in (_lib.COST_SAME, _lib.COST_FORCE_DIRECT, _lib.COST_FORCE_MFMA, _lib.COST_PARTIAL_ONLY, _lib.COST_GRAM_SUMS_ONLY,
                  _lib.COST_FROM_GRAM_SUMS, _lib.COST_BICAUSAL_TERM_ONLY, _lib.COST_CAUSAL_ADD, _lib.MIXED_CMIX_GIVEN):
        assert call(R | other) == _lib.EINVAL, other
        assert b"no other flag" in lib.kccot_last_error()
    assert call(R, C=None) == _lib.EINVAL and call(R, ws=None) == _lib.EINVAL
    for kw in ({"Bx": 0}, {"By": 0}, {"Bx": -3}, {"By": -1}, {"sc": 0.0}, {"sc": -0.5}, {"sc": float("nan")}, {"ws": 20}):
        assert call(R, **kw) == _lib.EINVAL, kw
    assert call(R, wsb=need - 1) == _lib.EWORKSPACE and call(R, wsb=0) == _lib.EWORKSPACE
    assert call(R, Bx=65535 * 4 + 1, By=1) == _lib.EUNSUPPORTED
    # the stated workspace covers the doubles the call touches at every shape of the tests and at extreme aspect ratios
    for Bx, By in ((1, 1), (5, 37), (16, 16), (64, 64), (32, 256), (64, 512), (1, 100000), (100000, 1), (3, 65), (4096, 4096)):
        tiles = ((Bx + 3) // 4) * ((By + 63) // 64)
        assert int(lib.kccot_pairwise_cost_workspace_bytes(Bx, By, 1)) >= 8 * (1 + tiles), (Bx, By)
    # the three-matrix entry and the loss entry points refuse it
    def refused(rc):
        return rc == _lib.EINVAL and b"RBF_SUM" in lib.kccot_last_error()

    assert refused(lib.kccot_pairwise_cost3_f32(one, one, 8, 64, 0.5, None, None, None, None, 1, 1, R, one, one, 1 << 20, None))
    loss_args = (one, one, 8, 256, 0.5, one, one, one, one, 4, 2, 1.0, 100, 100, 0.01, R)
    #                                                  C3   u_hist v_hist cost3 nits loss ticket ws
    assert refused(lib.kccot_sinkhorn_loss_fwd_f32(*loss_args, one, one, one, one, one, one, one, one, 1 << 30, None))
    #                                                        C3   dC3u cost3 nits loss ticket ws
    assert refused(lib.kccot_sinkhorn_loss_fused_fwd_f32(*loss_args, one, one, one, one, one, one, one, 1 << 30, None))
    #                                                           C3   u_hist v_hist dC3u cost3 nits loss ticket ws
    assert refused(lib.kccot_bicausal_sinkhorn_loss_fwd_f32(*loss_args, one, None, None, one, one, one, one, one, one, 1 << 30,
                                                            None))
    #                                                        Cmix u_hist v_hist dCmixu cost4 nits loss ticket ws
    assert refused(lib.kccot_mixed_sinkhorn_loss_fwd_f32(one, one, 8, 256, 0.5, *([one] * 6), 4, 2, 1.0, 100, 100, 0.01, R,
                                                         one, None, None, one, one, one, one, one, one, 1 << 30, None))
