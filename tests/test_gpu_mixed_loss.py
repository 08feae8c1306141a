"""GPU tests of compute_mixed_sinkhorn_loss (the two-minibatch Sinkhorn divergence, an extension of the reference):
against the fixtures written by tests/golden/make_mixed_golden.py (the reference's own compute_sinkhorn per term), fp64
torch autograd of the oracle composition, the one-batch loss in the identity case, the n > 128 solver, graph replay.

Tolerances follow tests/test_gpu_parity.py: costs 5e-5 (fp32 fixture) / 1e-4 (fp64) relative, cost matrices 1e-5 of
max|C|, iteration counts identical, gradients max(2.5e-5, 4 x the oracle's own fp32 / fp64 gap of the case) of max|grad|.
The loss (W1 + W2) - W3 - W4 of two INDEPENDENT minibatches can cancel to 1e-3 of its terms (far regime), so its 1e-4
bound is taken relative to max(|loss|, max_k |W_k|): exactly the relative bound wherever the loss does not cancel."""
import json
import os

import numpy as np
import pytest
import torch

import cases
import mixed_cases
from oracle import gan_utils_torch as ot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
GRAD_GAP = json.load(open(os.path.join(GOLD, "grad_gap.json")))["gaps"]
WRT = ["fake", "fake_p", "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p"]
SMALL = [c for c in mixed_cases.CASES if c[0] != "cfg2"]


@pytest.fixture(scope="module")
def G():
    from kccotgan_amd import gan_utils
    return gan_utils


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _reset_flags(G, L):
    defaults = {k: L.get_option(k) for k in L.option_names()}
    yield
    G.cost_flags = 0
    for k, v in defaults.items():
        L.set_option(k, v)


def load(shape, seed, regime):
    g = np.load(os.path.join(GOLD, mixed_cases.case_name(shape, seed, regime) + ".npz"))
    inp = mixed_cases.gen_inputs(shape, seed, regime)
    np.testing.assert_array_equal(mixed_cases.checksum(inp), g["checksum"])
    return g, inp, {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def grad_tol(shape, seed, regime):
    gaps = GRAD_GAP.get(cases.case_name(shape, seed, regime), {})
    return max(2.5e-5, 4.0 * max(gaps.values(), default=0.0))


def call(G, t, **kw):
    return G.compute_mixed_sinkhorn_loss(t["real"], t["fake"], t["real_p"], t["fake_p"], cases.SC, 0.8, 100, t["h_fake"],
                                         t["m_real"], t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"], **kw)


def oracle(d, chunk=None):
    """torch composition of the reference's compute_sinkhorn over the four terms (fp64 or fp32 by the inputs)."""
    fl = lambda v: ot.flatten_video(v)
    w = [ot.compute_sinkhorn(fl(d[a]), fl(d[b]), d[h], d[m], cases.SC, chunk=chunk) for a, b, h, m, _ in mixed_cases.TERMS]
    return (w[0] + w[1]) - w[2] - w[3]


def loss_ok(got, g, sfx):
    scale = max(abs(float(g["loss" + sfx])), max(abs(float(g["w%d%s" % (t, sfx)])) for t in range(1, 5)))
    return abs(float(got.detach()) - float(g["loss" + sfx])) <= 1e-4 * scale


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape,seed,regime", mixed_cases.CASES)
def test_mixed_loss_matches_reference_terms(G, L, shape, seed, regime, fused):
    g, inp, t = load(shape, seed, regime)
    L.set_option("sinkhorn_fused", fused)
    t["fake"].requires_grad_(True)                 # a gradient wanted: the fused solve + sweep where eligible
    loss = call(G, t)
    assert G.last_info["compute_mixed_sinkhorn_loss_fused_sweep"] == bool(fused and L.lib.kccot_sinkhorn_fused_eligible(
        inp["real"].shape[0], 100))
    nits = G.last_info["compute_mixed_sinkhorn_loss"].cpu().numpy().tolist()
    assert nits == [int(g["nits%d" % k]) for k in range(1, 5)]
    costs = G.last_info["compute_mixed_sinkhorn_loss_costs"].cpu().numpy()
    Cmix = G.last_info["compute_mixed_sinkhorn_loss_Cmix"].cpu().numpy()
    for k in range(4):
        ref, ref64 = float(g["w%d" % (k + 1)]), float(g["w%d_f64" % (k + 1)])
        assert abs(costs[k] - ref) <= 5e-5 * abs(ref) and abs(costs[k] - ref64) <= 1e-4 * abs(ref64), (k, costs[k], ref)
        for sfx in ("", "_f64"):
            C = g["C%d%s" % (k + 1, sfx)]
            np.testing.assert_allclose(Cmix[k], C, rtol=0, atol=1e-5 * np.abs(C).max(), err_msg="C%d%s" % (k + 1, sfx))
    assert loss_ok(loss, g, "") and loss_ok(loss, g, "_f64"), (float(loss), float(g["loss"]))
    G.raise_if_solver_aborted(("compute_mixed_sinkhorn_loss",))


def test_mixed_loss_forward_only_and_eps_l_default(G, L):
    g, inp, t = load("small", 0, "near")
    a = call(G, t)                                                    # no gradient: history-free forward
    assert G.last_info["compute_mixed_sinkhorn_loss_fused_sweep"] is False
    b = G.compute_mixed_sinkhorn_loss(t["real"], t["fake"], t["real_p"], t["fake_p"], cases.SC, 0.1, 5, t["h_fake"],
                                      t["m_real"], t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"])
    assert float(a) == float(b)                                       # eps / L ignored by default (quirk 1)
    c = call(G, t, honor_eps_l=True)                                  # eps = 0.8, L = 100
    assert float(c) != float(a)
    assert loss_ok(a, g, "")


def _oracle_grads(inp, dtype, chunk=None):
    d = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in WRT:
        d[k].requires_grad_(True)
    val = oracle(d, chunk)
    return val, dict(zip(WRT, (x.double().numpy() for x in torch.autograd.grad(val, [d[k] for k in WRT]))))


def _check_grads(G, L, shape, seed, regime, fused, rows=None):
    """Tolerance rule of test_gpu_parity.py: max(floor, 4 x the oracle's own fp32 / fp64 autograd gap), here with the gap
    measured on THIS mixed case per gradient: W(x, x') and W(y, y') pair independent samples, so even a "near" case holds
    two sharp (far-regime) problems with their own conditioning."""
    g, inp, t = load(shape, seed, regime)
    L.set_option("sinkhorn_fused", fused)
    for k in WRT:
        t[k].requires_grad_(True)
    chunk = 8 if shape == "cfg2" else None
    ref_val, ref = _oracle_grads(inp, torch.float64, chunk)
    _, ref32 = _oracle_grads(inp, torch.float32, chunk)
    tols = {}
    for k in WRT:
        gap = float(np.abs(ref32[k] - ref[k]).max() / np.abs(ref[k]).max())
        tols[k] = max(grad_tol(shape, seed, regime), 4.0 * gap)
    loss = call(G, t)
    got = dict(zip(WRT, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in WRT]))))
    assert abs(float(loss) - float(ref_val)) <= 1e-4 * max(abs(float(ref_val)), abs(float(g["w1_f64"])),
                                                           abs(float(g["w3_f64"])), abs(float(g["w4_f64"])))
    for k in WRT:
        a, b = got[k], ref[k]
        if rows is not None and k in ("fake", "fake_p"):
            a, b = a[rows], b[rows]
        np.testing.assert_allclose(a, b, rtol=0, atol=tols[k] * np.abs(ref[k]).max(), err_msg=k)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("shape,seed,regime", SMALL)
def test_mixed_loss_gradients_match_fp64_autograd(G, L, shape, seed, regime, fused):
    _check_grads(G, L, shape, seed, regime, fused)


def test_mixed_loss_cfg2_gradients_sampled_rows(G, L):
    _check_grads(G, L, "cfg2", 0, "near", 1, rows=[0, 17, 63])


def test_identity_case_equals_the_one_batch_loss(G, L):
    g, inp, t = load("deci64", 0, "near")
    base = {k: t[k].clone().requires_grad_(True) for k in ("fake", "h_fake", "m_real", "m_fake")}
    h_real = torch.from_numpy(cases.gen_inputs("deci64", 0, "near")["h_real"]).to(DEV).requires_grad_(True)
    one = G.compute_sinkhorn_loss(t["real"], base["fake"], cases.SC, 0.8, 100, base["h_fake"], base["m_real"], h_real,
                                  base["m_fake"])
    dfake = torch.autograd.grad(one, [base["fake"]])[0]
    y = t["fake"].clone().requires_grad_(True)
    y_p = t["fake"].clone().requires_grad_(True)
    mix = G.compute_mixed_sinkhorn_loss(t["real"], y, t["real"], y_p, cases.SC, 0.8, 100, t["h_fake"], t["m_real"], h_real,
                                        t["m_fake"], t["h_fake"], t["m_real"])
    dy, dy_p = torch.autograd.grad(mix, [y, y_p])
    assert abs(float(mix) - float(one)) <= 1e-5 * abs(float(one))
    amax = float(dfake.abs().max())
    assert float((dy + dy_p - dfake).abs().max()) <= 1e-5 * amax


@pytest.mark.parametrize("fused", [1, 0])
def test_mixed_loss_errors(G, L, fused):
    g, inp, t = load("tiny", 0, "near")
    L.set_option("sinkhorn_fused", fused)
    r = t["real"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        G.compute_mixed_sinkhorn_loss(r, t["fake"], t["real_p"], t["fake_p"], cases.SC, 0.8, 100, t["h_fake"], t["m_real"],
                                      t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"])
    with pytest.raises(ValueError):
        G.compute_mixed_sinkhorn_loss(t["real"], t["fake"][:-1], t["real_p"], t["fake_p"], cases.SC, 0.8, 100, t["h_fake"],
                                      t["m_real"], t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"])
    with pytest.raises(ValueError):
        G.compute_mixed_sinkhorn_loss(t["real"], t["fake"], t["real_p"], t["fake_p"], cases.SC, 0.8, 100, t["h_fake"][:, 1:],
                                      t["m_real"], t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"])


def test_large_batch_runs_the_four_problem_multi_cu_path(G, L):
    """deci256: n = 256 > 128, the four solves on the multi-CU (or streaming) solver, the history path both ways."""
    B, H, T, W, C, J = cases.SHAPES["deci256"]
    rng = np.random.default_rng(2024)
    inp = {}
    for k in ("real", "real_p"):
        inp[k] = rng.random((B, H, T, W, C), dtype=np.float32)
    for k, src in (("fake", "real"), ("fake_p", "real_p")):
        inp[k] = np.clip(inp[src] + np.float32(0.05) * rng.standard_normal((B, H, T, W, C), dtype=np.float32), 0, 1).astype(np.float32)
    for k in ("h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p"):
        inp[k] = rng.random((B, T, J), dtype=np.float32)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    for k in WRT:
        d[k].requires_grad_(True)
        t[k].requires_grad_(True)
    ref_val = oracle(d)
    ref = dict(zip(WRT, (x.numpy() for x in torch.autograd.grad(ref_val, [d[k] for k in WRT]))))
    loss = call(G, t)
    assert G.last_info["compute_mixed_sinkhorn_loss_fused_sweep"] is False
    G.raise_if_solver_aborted(("compute_mixed_sinkhorn_loss",))
    got = dict(zip(WRT, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in WRT]))))
    assert abs(float(loss) - float(ref_val)) <= 1e-4 * abs(float(ref_val)), (float(loss), float(ref_val))
    for k in WRT:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-4 * np.abs(ref[k]).max(), err_msg=k)


@pytest.mark.parametrize("fused", [1, 0])
def test_mixed_loss_graph_replay_is_bit_identical(G, L, fused):
    g, inp, t = load("deci64", 0, "near")
    L.set_option("sinkhorn_fused", fused)
    L.set_option("sinkhorn_shortcut", 0)
    for k in WRT:
        t[k].requires_grad_(True)

    def step():
        loss = call(G, t)
        return [loss.detach().clone()] + [x.clone() for x in torch.autograd.grad(loss, [t[k] for k in WRT])]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for rewrite in range(3):
        if rewrite:
            rng = np.random.default_rng(100 + rewrite)
            with torch.no_grad():
                for k in ("fake", "fake_p", "real_p", "h_fake_p"):
                    t[k].copy_(torch.from_numpy(np.clip(inp[k] + np.float32(0.01) * rng.standard_normal(inp[k].shape,
                                                                                              dtype=np.float32), 0, 1)))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)
