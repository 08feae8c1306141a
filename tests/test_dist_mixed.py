"""The batch-sharded mixed Sinkhorn divergence (kccotgan_amd.dist.sharded_mixed_sinkhorn_loss) over gloo.

CPU: world sizes 2 and 4 with the torch oracle as the compute ops (tests/dist_mixed_worker.py), in both regimes (whole Cmix
on every rank; row blocks of the stacked problem, forced with KCCOT_DIST_ROW_BLOCKS=1), against the single-process fp64
composition (W1 + W2) - W3 - W4 of compute_sinkhorn; the refusals before any collective; the two new ABI flags' refusals.
GPU (-m gpu): two ranks (four at B = 256) sharing cuda:0 with the HIP library, against the single-GPU
compute_mixed_sinkhorn_loss and fp64 autograd of the oracle composition, with the graph-captured step.  The workers are
the only processes this file starts on the GPU: rank 0 evaluates the single-GPU reference itself, and this process never
touches the device (it may still hold the idle context of earlier GPU tests of the session: at four ranks that makes five
processes with the device open, within the machine's limit of 16)."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import cases
import mixed_cases
from oracle import gan_utils_torch as ot

HERE = os.path.dirname(os.path.abspath(__file__))
WRT = ("fake", "fake_p", "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")
GRAD_TOL_FACTOR, GRAD_TOL_FLOOR = 4.0, 2.5e-5          # the single-GPU rule of tests/test_gpu_parity.py
ROWS = {"KCCOT_DIST_ROW_BLOCKS": "1"}
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
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_mixed_worker.py"), str(r), str(world), str(port),
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
    """(W1 + W2) - W3 - W4 with W = ot.compute_sinkhorn (epsilon 1, L 100: what the loss runs), the four W, and the
    gradients w.r.t. WRT by autograd in `dtype`."""
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in WRT:
        t[k].requires_grad_(True)
    fl = ot.flatten_video
    w = [ot.compute_sinkhorn(fl(t[a]), fl(t[b]), t[h], t[m], cases.SC, chunk=32) for a, b, h, m, _ in mixed_cases.TERMS]
    loss = ((w[0] + w[1]) - w[2]) - w[3]
    grads = torch.autograd.grad(loss, [t[k] for k in WRT])
    return float(loss), [float(x) for x in w], [g.double().numpy() for g in grads]


def oracle(shape, seed, regime, world):
    """fp64 loss, W_k and gradients of the composition on the whole batch, and the tolerance per gradient: max(2.5e-5,
    4 x the composition's own fp32-vs-fp64 gap) relative to max|grad| -- the parity rule of the single-GPU tests."""
    key = (shape, seed, regime, world)
    if key not in _ORACLE:
        import dist_mixed_worker as w
        inp = w.batch(shape, seed, regime, world)
        l64, w64, g64 = composition(inp, torch.float64)
        _, _, g32 = composition(inp, torch.float32)
        tol = {k: max(GRAD_TOL_FLOOR, GRAD_TOL_FACTOR * float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-30)))
               for k, a, b in zip(WRT, g64, g32)}
        _ORACLE[key] = (l64, w64, dict(zip(WRT, g64)), tol)
    return _ORACLE[key]


def _rows(g, r, Bl):
    return g.reshape(g.shape[0], -1)[r * Bl:(r + 1) * Bl]


# ---------------------------------------------------------------------------------------------------- CPU (gloo)
@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("shape,seed,regime,rows", [("tiny", 0, "near", False), ("small", 0, "near", False),
                                                     ("small", 0, "near", True), ("small", 1, "far", False),
                                                     ("small", 1, "far", True), ("deci64", 0, "near", False),
                                                     ("deci64", 0, "near", True)])
def test_sharded_mixed_equals_single_process_oracle(world, shape, seed, regime, rows, tmp_path):
    """Both regimes (tiny: K < 256, row blocks by default; small / deci64: whole Cmix by default, row blocks forced): the
    stacked gathers, the two row-block calls and the block map, the causal adds, the exchange of the row blocks, the
    replicated solves and each rank's gradient rows of y, y' and the six features, against the fp64 composition."""
    import dist_mixed_worker as w
    res = launch(world, shape, seed, regime, "cpu", "oracle", tmp_path, ROWS if rows else None)
    ref, _, grads = composition(w.batch(shape, seed, regime, world), torch.float64)
    B = grads[0].shape[0]
    Bl = B // world
    for r, out in enumerate(res):
        assert abs(float(out["loss"]) - ref) <= 1e-10 * abs(ref)        # the GLOBAL loss, identical on every rank
        assert float(out["loss"]) == float(res[0]["loss"])
        for k, g in zip(WRT, grads):
            np.testing.assert_allclose(_rows(out["d" + k], 0, Bl), _rows(g, r, Bl), rtol=0,
                                       atol=1e-9 * max(np.abs(g).max(), 1e-30), err_msg=k)


def _shards():
    from kccotgan_amd import dist as kd
    t = {k: torch.from_numpy(v).double() for k, v in mixed_cases.gen_inputs("small", 0, "near").items()}
    return t, kd


def _call(kd, t, **kw):
    return kd.sharded_mixed_sinkhorn_loss(t["real"], t["fake"], t["real_p"], t["fake_p"], cases.SC,
                                          *(t[k] for k in mixed_cases.KEYS[4:]), **kw)


def test_sharded_mixed_refuses_before_any_collective():
    """No process group exists here: every refusal must come before the first collective, with a message that names it."""
    from dist_mixed_worker import MixedOracleOps
    from dist_worker import OracleOps
    t, kd = _shards()
    with pytest.raises(NotImplementedError, match="mixed_loss_full"):            # ops without the mixed operations
        _call(kd, t, ops=OracleOps)
    with pytest.raises(NotImplementedError, match="ksplit"):
        _call(kd, t, ops=MixedOracleOps, protocol="ksplit")
    with pytest.raises(ValueError, match="protocol"):
        _call(kd, t, ops=MixedOracleOps, protocol="chunks")
    bad = dict(t, fake_p=t["fake_p"][:-1])
    with pytest.raises(ValueError, match="video"):
        _call(kd, bad, ops=MixedOracleOps)
    bad = dict(t, m_real_p=t["m_real_p"][:, :-1])
    with pytest.raises(ValueError, match="feature"):
        _call(kd, bad, ops=MixedOracleOps)
    bad = dict(t, real_p=t["real_p"].clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="real"):
        _call(kd, bad, ops=MixedOracleOps)
    assert set(kd.MIXED_OPS) <= set(dir(kd.HipOps)) and set(kd.MIXED_OPS) <= set(dir(MixedOracleOps))


def test_public_signature_and_trainer_refusal():
    import inspect
    from kccotgan_amd import dist as kd
    from kccotgan_amd.kernel_train import KCCOTTrainer
    sig = inspect.signature(kd.sharded_mixed_sinkhorn_loss)
    assert list(sig.parameters) == ["f_real_l", "f_fake_l", "f_real_p_l", "f_fake_p_l", "scaling_coef", "h_fake_l", "m_real_l",
                                    "h_real_p_l", "m_fake_l", "h_fake_p_l", "m_real_p_l", "group", "ops", "epsilon", "L",
                                    "protocol"]
    assert list(inspect.signature(kd.sharded_mixed_loss_step).parameters) == ["shard", "sc", "group", "epsilon", "L"]
    assert "GATHER_CHUNKS" in kd.sharded_mixed_sinkhorn_loss.__doc__
    with pytest.raises(NotImplementedError, match="mixed_sinkhorn") as e:
        KCCOTTrainer(2, device="cuda", mixed_sinkhorn=True, group=object())
    assert "sharded_mixed_sinkhorn_loss" in str(e.value)


def test_causal_add_and_cmix_given_flags_are_declared_and_refused_on_their_arguments():
    """KCCOT_COST_CAUSAL_ADD = 128 (kccot_pairwise_cost_f32) and KCCOT_MIXED_CMIX_GIVEN = 256
    (kccot_mixed_sinkhorn_loss_fwd_f32) in the header and the binding; with any other flag, without h / M / C_out / Cmix or
    with a bad shape the call is rejected on its arguments (no launch: this runs without a GPU)."""
    from kccotgan_amd import _lib
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "kccot.h")).read()
    assert re.search(r"#define KCCOT_COST_CAUSAL_ADD 128u", hdr)
    assert re.search(r"#define KCCOT_MIXED_CMIX_GIVEN 256u", hdr)
    assert _lib.COST_CAUSAL_ADD == 128 and _lib.MIXED_CMIX_GIVEN == 256
    lib, one = _lib.lib, 16
    others = (_lib.COST_SAME, _lib.COST_FORCE_DIRECT, _lib.COST_FORCE_MFMA, _lib.COST_PARTIAL_ONLY, _lib.COST_GRAM_SUMS_ONLY,
              _lib.COST_FROM_GRAM_SUMS, _lib.COST_BICAUSAL_TERM_ONLY)
    # ---- CAUSAL_ADD
    A = _lib.COST_CAUSAL_ADD

    def add(flags, Bx=8, By=9, h=one, M=one, C=one, t=3, j=2, h2=None, M2=None):
        return lib.kccot_pairwise_cost_f32(None, None, Bx, By, 0, 0.5, h, M, h2, M2, t, j, flags, C, None, 0, None)

    for other in others + (_lib.MIXED_CMIX_GIVEN,):
        assert add(A | other) == _lib.EINVAL, other
        assert b"no other flag" in lib.kccot_last_error()
    assert add(A, h=None) == _lib.EINVAL and add(A, M=None) == _lib.EINVAL and add(A, C=None) == _lib.EINVAL
    assert add(A, h2=one, M2=one) == _lib.EINVAL
    for kw in ({"Bx": 0}, {"By": 0}, {"Bx": -3}, {"t": 0}, {"j": 0}):
        assert add(A, **kw) == _lib.EINVAL, kw
    assert add(A, Bx=65535 * 16 + 1) == _lib.EUNSUPPORTED
    # the cost3 entry and the mixed loss's cost stage refuse it
    assert lib.kccot_pairwise_cost3_f32(one, one, 8, 64, 0.5, None, None, None, None, 1, 1, A, one, one, 1 << 20,
                                        None) == _lib.EINVAL
    # ---- CMIX_GIVEN
    G = _lib.MIXED_CMIX_GIVEN

    def given(flags, B=8, Cmix=one, eps=1.0, L=100, uh=None, vh=None, dCu=one, ticket=one, costs=one):
        return lib.kccot_mixed_sinkhorn_loss_fwd_f32(None, None, B, 0, 0.5, *([None] * 6), 1, 1, eps, L, 100, 0.01, flags,
                                                     Cmix, uh, vh, dCu, costs, one, one, ticket, None, 0, None)

    for other in others + (A,):
        assert given(G | other) == _lib.EINVAL, other
        assert b"no other flag" in lib.kccot_last_error()
    assert given(G, Cmix=None) == _lib.EINVAL and given(G, costs=None) == _lib.EINVAL
    for kw in ({"B": 0}, {"B": -1}, {"B": (1 << 19) + 1}, {"eps": 0.0}, {"L": -1}):
        assert given(G, **kw) == _lib.EINVAL, kw
    assert given(G, uh=one, vh=one) == _lib.EINVAL         # history and dCmix_unit together
    assert given(G, ticket=None) == _lib.EINVAL            # the fused mode needs the ticket
    # without the flag the videos and features are still required
    assert given(0) == _lib.EINVAL and b"null input" in lib.kccot_last_error()
    # the history mode's workspace (n > 128: the streaming solvers need one) is checked before any launch
    need = lib.kccot_sinkhorn_workspace_bytes(4, 256)
    assert need > 0
    assert given(G, B=256, dCu=None, uh=one, vh=one) == _lib.EWORKSPACE


# ---------------------------------------------------------------------------------------------------- GPU (HIP, gloo)
def _check_hip(res, shape, seed, regime, world, replicated):
    """Against the single-GPU loss (rank 0 evaluated it on the whole batch, in its own process) and the fp64 oracle, with
    the tolerances of DESIGN.md section 10.  replicated: Cmix, loss and iteration counts bit-identical to the single GPU."""
    l64, w64, g64, tol = oracle(shape, seed, regime, world)
    ref = res[0]
    B = ref["ref_Cmix"].shape[1]
    Bl = B // world
    scale = max(abs(l64), max(abs(x) for x in w64))
    for r, out in enumerate(res):
        assert float(out["loss"]) == float(ref["loss"])                          # the same loss on every rank
        assert np.array_equal(out["Cmix"].view(np.int32), ref["Cmix"].view(np.int32))
        assert abs(float(out["loss"]) - l64) <= 1e-4 * scale, (float(out["loss"]), l64)
        assert bool(out["nits_is_sharded"]) and bool(out["graphed_sees_new_inputs"])
        # the graph-captured step runs the eager step's kernels on the same operands
        assert bool(out["graphed_loss_equal"]) and bool(out["graphed_grads_equal"])
        assert bool(out["graphed_replicated"]) == replicated
        for k in WRT:
            got = _rows(out["d" + k], 0, Bl)
            g1, scale_k = ref["ref_d" + k], np.abs(g64[k]).max()
            # the parity rule -- or, where the single-GPU loss on the same batch is itself farther from fp64 than that (the
            # n = 256 solves: its own tests hold it to 1e-4, tests/test_gpu_mixed_loss.py), no more than 1.25 x its distance
            single = float(np.abs(g1 - g64[k]).max()) / scale_k
            sharded = float(np.abs(got - _rows(g64[k], r, Bl)).max()) / scale_k
            print("%s rank %d %s: sharded %.2e, single GPU %.2e of max|grad| from fp64 (parity tol %.2e)"
                  % (shape, r, k, sharded, single, tol[k]))
            bound = max(tol[k], 1.25 * single)
            assert sharded <= bound, "%s vs fp64 oracle: %.2e > %.2e (single GPU %.2e)" % (k, sharded, bound, single)
            # HIP against HIP: two fp32 evaluations, each within its bound of fp64
            np.testing.assert_allclose(got, _rows(g1, r, Bl), rtol=0, atol=2.0 * bound * scale_k, err_msg="%s vs single GPU" % k)
    C1 = ref["ref_Cmix"]
    if replicated:
        assert np.array_equal(ref["Cmix"].view(np.int32), C1.view(np.int32)), "Cmix differs from the single-GPU loss's"
        assert float(ref["loss"]) == float(ref["ref_loss"])
        assert np.array_equal(ref["nits"], ref["ref_nits"])
        # the feature gradients come from the single-GPU loss's own backward call on the same operands: its rows, bit for bit
        Bl = B // world
        for r, out in enumerate(res):
            for k in WRT[2:]:
                assert np.array_equal(_rows(out["d" + k], 0, Bl), _rows(ref["ref_d" + k], r, Bl)), (r, k)
    else:
        np.testing.assert_allclose(ref["Cmix"], C1, rtol=0, atol=1e-5 * np.abs(C1).max())


@pytest.mark.gpu
@pytest.mark.parametrize("shape,world,rows,replicated", [
    ("deci64", 2, False, True),          # whole Cmix: the single-GPU loss call on every rank
    ("deci64", 2, True, False),          # forced rows: Bl = 32, the matrix pipe at 2B = 128
    ("deci64@40", 2, False, True),       # ragged, replicated by default
    ("deci64@40", 2, True, False),       # ragged rows: the direct kernel at 2B = 80
    ("deci128", 2, False, False),        # Bl = 64, the matrix pipe at 2B = 256
    ("deci256", 2, False, False),        # Bl = 128: the direct rows kernel; n = 256: the multi-CU solver
    ("deci256", 4, False, False),        # Bl = 64: the matrix pipe at 2B = 512 (four worker processes on the GPU)
])
def test_sharded_mixed_hip(shape, world, rows, replicated, tmp_path):
    res = launch(world, shape, 0, "near", "cuda:0", "hip", tmp_path, ROWS if rows else None)
    _check_hip(res, shape, 0, "near", world, replicated)


@pytest.mark.gpu
def test_row_regime_cmix_equals_the_single_gpu_cmix_when_the_videos_are_zero(tmp_path):
    """All four videos zero: every distance is exactly 0 on both routes, so the row-regime Cmix holds the causal terms
    alone -- and KCCOT_COST_CAUSAL_ADD must sum them exactly as the single-GPU loss's finalize does: bit for bit."""
    res = launch(2, "deci64", 0, "near+zero", "cuda:0", "hip", tmp_path, ROWS)
    ref = res[0]
    assert not bool(ref["graphed_replicated"])
    assert np.abs(ref["ref_Cmix"]).max() > 0
    assert np.array_equal(ref["Cmix"].view(np.int32), ref["ref_Cmix"].view(np.int32))
    assert float(ref["loss"]) == float(ref["ref_loss"]) and np.array_equal(ref["nits"], ref["ref_nits"])
