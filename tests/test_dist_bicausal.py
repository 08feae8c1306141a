"""The batch-sharded bi-causal Sinkhorn loss (kccotgan_amd.dist.sharded_bicausal_sinkhorn_loss) over gloo.

CPU: world sizes 2 and 4 with the torch oracle as the compute ops (tests/dist_bicausal_worker.py) against the
single-process fp64 composition 2 W_xy - W_xx - W_yy of compute_sinkhorn(..., bi_causal=True).
GPU (-m gpu): two ranks sharing cuda:0 with the HIP library, against the single-GPU compute_bicausal_sinkhorn_loss and
fp64 autograd of the oracle composition; the graph-captured steps; one data-parallel trainer iteration."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import bicausal_cases
import cases
from oracle import gan_utils_torch as ot

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("fake", "h_fake", "h_real", "m_real", "m_fake")
GRAD_TOL_FACTOR, GRAD_TOL_FLOOR = 4.0, 2.5e-5          # the single-GPU rule of tests/test_gpu_parity.py
_ORACLE = {}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(world, shape, seed, regime, device, mode, tmp_path, env=None):
    port = free_port()
    out = os.path.join(str(tmp_path), "rank%d.npz")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_bicausal_worker.py"), str(r), str(world), str(port),
                               shape, str(seed), regime, device, mode, out], env=dict(os.environ, **(env or {})))
             for r in range(world)]
    try:
        for p in procs:
            assert p.wait(timeout=600) == 0
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [np.load(out % r) for r in range(world)]


def composition(inp, dtype):
    """2 W_xy - W_xx - W_yy with W = ot.compute_sinkhorn(..., bi_causal=True) (epsilon 1, L 100: what the loss runs) and
    its gradients w.r.t. the five differentiated inputs, by autograd in `dtype`."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    d = dict(t, real=ot.flatten_video(t["real"]), fake=ot.flatten_video(t["fake"]))
    w = {tag: ot.compute_sinkhorn(d[a], d[b], d[hy], d[mx], cases.SC, hx=d[hx], My=d[my], bi_causal=True)
         for tag, a, b, hy, mx, hx, my in bicausal_cases.TERMS}
    loss = sum(bicausal_cases.WEIGHTS[tag] * w[tag] for tag in w)
    grads = torch.autograd.grad(loss, [t[k] for k in NAMES])
    return float(loss), [g.double().numpy() for g in grads]


def oracle(shape, seed, regime, world=2):
    """fp64 loss and gradients of the composition on the whole batch, and the tolerance per gradient: max(2.5e-5,
    4 x the composition's own fp32-vs-fp64 gap) relative to max|grad| -- the parity rule of the single-GPU tests."""
    key = (shape, seed, regime, world)
    if key not in _ORACLE:
        import dist_bicausal_worker as w
        inp = w.batch(shape, seed, regime, world)
        l64, g64 = composition(inp, torch.float64)
        _, g32 = composition(inp, torch.float32)
        tol = {k: max(GRAD_TOL_FLOOR, GRAD_TOL_FACTOR * float(np.abs(a - b).max() / np.abs(a).max()))
               for k, a, b in zip(NAMES, g64, g32)}
        _ORACLE[key] = (l64, dict(zip(NAMES, g64)), tol)
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------- CPU (gloo)
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("shape,seed,regime", [("small", 0, "near"), ("small", 1, "far"), ("tiny", 0, "near"),
                                                ("tiny", 1, "far")])
def test_sharded_bicausal_equals_single_process_oracle(world, shape, seed, regime, tmp_path):
    """Row blocks of the one-batch costs on every rank, all-gathered, the second causal terms added to the replicated
    C3, the replicated solves, each rank's gradient rows: against the fp64 composition of the whole batch."""
    import dist_bicausal_worker as w
    res = launch(world, shape, seed, regime, "cpu", "oracle", tmp_path)
    ref, grads = composition(w.batch(shape, seed, regime, world), torch.float64)
    B = grads[0].shape[0]
    Bl = B // world
    for r, out in enumerate(res):
        assert abs(float(out["loss"]) - ref) <= 1e-10 * abs(ref)        # the GLOBAL loss, identical on every rank
        assert float(out["loss"]) == float(res[0]["loss"])
        for k, g in zip(NAMES, grads):
            want = g.reshape(B, -1)[r * Bl:(r + 1) * Bl]
            np.testing.assert_allclose(out["d" + k].reshape(Bl, -1), want, rtol=0, atol=1e-9 * max(np.abs(g).max(), 1e-30),
                                       err_msg=k)


def test_sharded_bicausal_refuses_ops_without_the_bicausal_operations():
    """Injected ops without bicausal_term / bicausal_feature_grads: a clear refusal before any collective."""
    from dist_worker import OracleOps
    from kccotgan_amd import dist as kd
    t = {k: torch.from_numpy(v).double() for k, v in cases.gen_inputs("small", 0, "near").items()}
    with pytest.raises(NotImplementedError, match="bicausal_term"):
        kd.sharded_bicausal_sinkhorn_loss(t["real"], t["fake"], cases.SC, t["h_fake"], t["m_real"], t["h_real"], t["m_fake"],
                                          ops=OracleOps)


def test_trainer_refuses_sharded_bicausal_off_the_gpu():
    """The sharded bi-causal loss runs on the HIP library only: a data-parallel bi-causal trainer on the CPU is refused
    with a message that says so, before any collective."""
    from kccotgan_amd.kernel_train import KCCOTTrainer
    with pytest.raises(NotImplementedError, match="GPU only"):
        KCCOTTrainer(2, device="cpu", bi_causal=True, group=object())
    with pytest.raises(NotImplementedError, match="mixed_sinkhorn"):
        KCCOTTrainer(2, device="cuda", mixed_sinkhorn=True, group=object())


def test_term_only_flag_is_declared_and_refuses_every_other_flag():
    """KCCOT_COST_BICAUSAL_TERM_ONLY = 64 in the header and the binding; with any other cost flag, without a feature
    tensor, without C3 or with a bad shape the call is rejected on its arguments (no launch: this runs without a GPU);
    the loss entry points refuse the flag."""
    import re
    from kccotgan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "kccot.h")).read()
    assert re.search(r"#define KCCOT_COST_BICAUSAL_TERM_ONLY 64u", hdr)
    assert _lib.COST_BICAUSAL_TERM_ONLY == 64
    lib, T, one = _lib.lib, _lib.COST_BICAUSAL_TERM_ONLY, 16
    f = (one, one, one, one)
    call = lambda flags, B=8, feats=f, C3=one, t=3, j=2: lib.kccot_pairwise_cost3_f32(None, None, B, 0, 0.5, *feats, t, j, flags,
                                                                                      C3, None, 0, None)
    for other in (_lib.COST_SAME, _lib.COST_FORCE_DIRECT, _lib.COST_FORCE_MFMA, _lib.COST_PARTIAL_ONLY,
                  _lib.COST_GRAM_SUMS_ONLY, _lib.COST_FROM_GRAM_SUMS):
        assert call(T | other) == _lib.EINVAL, other
        assert b"no other flag" in lib.kccot_last_error()
    for i in range(4):
        assert call(T, feats=tuple(None if q == i else p for q, p in enumerate(f))) == _lib.EINVAL
    assert call(T, C3=None) == _lib.EINVAL
    assert call(T, B=0) == _lib.EINVAL and call(T, t=0) == _lib.EINVAL and call(T, j=0) == _lib.EINVAL
    assert call(T, B=65535 * 8 + 1) == _lib.EUNSUPPORTED
    ws = lib.kccot_bicausal_sinkhorn_loss_workspace_bytes(8, 64)
    assert lib.kccot_sinkhorn_loss_fwd_f32(one, one, 8, 64, 0.5, *f, 3, 2, 1.0, 100, 100, 0.01, T, one, None, None, one, one,
                                           one, one, one, ws, None) == _lib.EINVAL
    assert lib.kccot_bicausal_sinkhorn_loss_fwd_f32(one, one, 8, 64, 0.5, *f, 3, 2, 1.0, 100, 100, 0.01, T, one, None, None,
                                                    one, one, one, one, one, one, ws, None) == _lib.EINVAL
    assert b"TERM_ONLY" in lib.kccot_last_error()


# ---------------------------------------------------------------------------------------------------- GPU (HIP, gloo)
def _single_gpu(inp):
    """compute_bicausal_sinkhorn_loss on the whole batch, one GPU: loss, gradients, C3, iteration counts."""
    from kccotgan_amd import gan_utils as G
    t = {k: torch.from_numpy(v).to("cuda:0") for k, v in inp.items()}
    for k in NAMES:
        t[k].requires_grad_(True)
    loss = G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"], cases.SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                            t["m_fake"])
    tag = "compute_bicausal_sinkhorn_loss"
    C3, nits = G.last_info[tag + "_C3"].cpu().numpy().copy(), G.last_info[tag].cpu().numpy().copy()
    grads = [g.cpu().double().numpy() for g in torch.autograd.grad(loss, [t[k] for k in NAMES])]
    return float(loss), grads, C3, nits


def _check_hip(res, shape, seed, regime, loss_rtol, world=2, graphed_exact=True):
    import dist_bicausal_worker as w
    inp = w.batch(shape, seed, regime, world)
    ref, grads, C3, nits = _single_gpu(inp)
    l64, g64, tol = oracle(shape, seed, regime, world)
    B = grads[0].shape[0]
    Bl = B // world
    for r, out in enumerate(res):
        assert abs(float(out["loss"]) - ref) <= loss_rtol * abs(ref), (float(out["loss"]), ref)
        assert float(out["loss"]) == float(res[0]["loss"])
        assert abs(float(out["loss"]) - l64) <= 1e-4 * abs(l64)
        assert bool(out["graphed_sees_new_inputs"])
        if graphed_exact:                    # the graph-captured step runs the eager step's kernels on the same operands
            assert bool(out["graphed_loss_equal"]) and bool(out["graphed_grads_equal"])
        for k, g in zip(NAMES, grads):
            got = out["d" + k].reshape(Bl, -1)
            # HIP against HIP: two fp32 evaluations, each within the oracle's tolerance of fp64
            np.testing.assert_allclose(got, g.reshape(B, -1)[r * Bl:(r + 1) * Bl], rtol=0, atol=2.0 * tol[k] * np.abs(g).max(),
                                       err_msg="%s vs single GPU" % k)
            np.testing.assert_allclose(got, g64[k].reshape(B, -1)[r * Bl:(r + 1) * Bl], rtol=0,
                                       atol=tol[k] * np.abs(g64[k]).max(), err_msg="%s vs fp64 oracle (tol %.2e)" % (k, tol[k]))
    return C3, nits


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["deci64", "cfg2"])
def test_sharded_bicausal_replicated_equals_single_gpu(shape, tmp_path):
    """B <= 64: every rank assembles the whole one-batch C3 and adds the term -- the single-GPU loss's kernels, so C3 is
    bit-identical to the single-GPU call's and so are the iteration counts."""
    res = launch(2, shape, 0, "near", "cuda:0", "hip", tmp_path)
    C3, nits = _check_hip(res, shape, 0, "near", 2e-6)
    for out in res:
        assert np.array_equal(out["C3"].view(np.int32), C3.view(np.int32)), "C3 differs from the single-GPU loss's"
        assert np.array_equal(out["nits"], nits) and bool(out["nits_is_sharded"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,protocol", [("deci128", "gather"), ("deci128", "gather_direct"), ("deci128", "gather_chunks"),
                                            ("deci128", "ksplit"), ("deci256", "gather"), ("deci256", "ksplit")])
def test_sharded_bicausal_row_blocks_and_ksplit(shape, protocol, tmp_path):
    """B = 128: row blocks on the matrix pipe (`gather`), on the direct kernel (KCCOT_DIST_ROWS=direct), over a chunked
    video gather (KCCOT_DIST_GATHER_CHUNKS=3), and the contraction-sharded protocol; B = 256: the multi-CU solver.  The
    term is added to the replicated C3 after the exchange, the feature gradients come from one cost backward per term."""
    env = {"gather": {"KCCOT_DIST_PROTOCOL": "gather"},
           "gather_direct": {"KCCOT_DIST_PROTOCOL": "gather", "KCCOT_DIST_ROWS": "direct"},
           "gather_chunks": {"KCCOT_DIST_PROTOCOL": "gather", "KCCOT_DIST_GATHER_CHUNKS": "3"},
           "ksplit": {"KCCOT_DIST_PROTOCOL": "ksplit"}}[protocol]
    res = launch(2, shape, 0, "near", "cuda:0", "hip", tmp_path, env=env)
    # GraphedShardedStep has no chunked video gather: it builds the whole-K row block, so its bits differ from the eager
    # chunked Gram sums (as for the one-batch loss, tests/test_dist_gloo.py::test_sharded_hip_batch_128)
    _check_hip(res, shape, 0, "near", 5e-6, graphed_exact=protocol != "gather_chunks")


@pytest.mark.gpu
def test_data_parallel_bicausal_trainer_keeps_replicas_identical(tmp_path):
    """Two ranks (gloo, one GPU), one KCCOTTrainer(bi_causal=True) iteration each on its half of a batch of four: the
    step ran the sharded bi-causal loss over the global batch, both replicas hold bit-identical weights before and after,
    the weights move, both report the same finite loss and pM."""
    a, b = launch(2, "none", 3, "none", "cuda:0", "train", tmp_path)
    assert bool(a["ran_sharded"]) and bool(b["ran_sharded"]) and int(a["B"]) == 4
    assert np.array_equal(a["p0"], b["p0"]) and np.array_equal(a["p1"], b["p1"])
    assert not np.array_equal(a["p0"], a["p1"]) and np.isfinite(a["p1"]).all()
    assert float(a["loss"]) == float(b["loss"]) and float(a["pm"]) == float(b["pm"])
    assert np.isfinite(float(a["loss"])) and np.isfinite(float(a["pm"]))
