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


# ---------------------------------------------------------------- random decimated inputs: every dispatch path at 2B
def _oracle_flat(d, sc=cases.SC, eps=1.0, L=100, chunk=16):
    """The oracle composition of oracle() on [B,1,K] videos (cost_xy sums the last two axes): (loss, [W1..W4], [C1..C4])."""
    C = [ot.modified_cost(d[a], d[b], d[h], d[m], sc, chunk) for a, b, h, m, _ in mixed_cases.TERMS]
    w = [ot.sinkhorn_from_cost(c, eps, L)[0] for c in C]
    return (w[0] + w[1]) - w[2] - w[3], w, C


def _rand_inputs(B, K, T=8, J=8, seed=0, far=False):
    """x, x' uniform; y, y' 0.05 from them ("near": W1, W2 near, W3, W4 pair independent samples) or uniform ("far")."""
    rng = np.random.default_rng(3000 + B + seed)
    inp = {}
    for k in ("real", "real_p"):
        inp[k] = rng.random((B, 1, K), dtype=np.float32)
    for k, src in (("fake", "real"), ("fake_p", "real_p")):
        inp[k] = rng.random((B, 1, K), dtype=np.float32) if far else np.clip(
            inp[src] + np.float32(0.05) * rng.standard_normal((B, 1, K), dtype=np.float32), 0, 1).astype(np.float32)
    for k in ("h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p"):
        inp[k] = rng.random((B, T, J), dtype=np.float32)
    return inp


def _run(G, inp, wrt=WRT, sc=cases.SC, **kw):
    """The mixed loss on the GPU with gradients of `wrt`: (loss, {name: grad}, [nits, costs, Cmix], fused_sweep)."""
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    for k in wrt:
        t[k].requires_grad_(True)
    loss = G.compute_mixed_sinkhorn_loss(t["real"], t["fake"], t["real_p"], t["fake_p"], sc, 0.8, 100, t["h_fake"],
                                         t["m_real"], t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"], **kw)
    info = [G.last_info["compute_mixed_sinkhorn_loss" + s].clone() for s in ("", "_costs", "_Cmix")]
    fused = G.last_info["compute_mixed_sinkhorn_loss_fused_sweep"]
    G.raise_if_solver_aborted(("compute_mixed_sinkhorn_loss",))
    grads = dict(zip(wrt, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in wrt])))) if wrt else {}
    return float(loss), grads, info, fused


def _ref(inp, wrt=WRT, sc=cases.SC, **kw):
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    for k in wrt:
        d[k].requires_grad_(True)
    val, w, C = _oracle_flat(d, sc, **kw)
    grads = dict(zip(wrt, (x.numpy() for x in torch.autograd.grad(val, [d[k] for k in wrt])))) if wrt else {}
    return float(val), [float(x) for x in w], [c.detach().numpy() for c in C], grads


def _check_mix(got, ref, gtol=1e-4, loss_abs=0.0):
    """Cost matrices 1e-5 of max|C|, the four costs 1e-4 relative (+ 1e-5 of max|C_k|: W_k averages C_k, whose causal
    term can cancel its distances), loss 1e-4 of max(|loss|, max_k |W_k|) (+ loss_abs), gradients gtol of max|grad| (a
    gradient the oracle has as exactly zero -- T = 1 features -- must be exactly zero)."""
    loss, grads, (nits, costs, Cmix), _ = got
    ref_val, ref_w, ref_C, ref_g = ref
    Cmix, costs = Cmix.cpu().numpy(), costs.cpu().numpy()
    for k in range(4):
        np.testing.assert_allclose(Cmix[k], ref_C[k], rtol=0, atol=1e-5 * np.abs(ref_C[k]).max(), err_msg="C%d" % (k + 1))
        assert abs(costs[k] - ref_w[k]) <= 1e-4 * abs(ref_w[k]) + 1e-5 * np.abs(ref_C[k]).max(), (k, costs[k], ref_w[k])
    assert abs(loss - ref_val) <= 1e-4 * max(abs(ref_val), max(abs(x) for x in ref_w)) + loss_abs, (loss, ref_val)
    for k, b in ref_g.items():
        scale = np.abs(b).max()
        if scale == 0:
            assert np.abs(grads[k]).max() == 0, k
            continue
        np.testing.assert_allclose(grads[k], b, rtol=0, atol=gtol * scale, err_msg=k)


def _check_shape(G, L, B, K, opts=(), flags=0):
    for k, v in opts:
        L.set_option(k, v)
    G.cost_flags = flags
    inp = _rand_inputs(B, K)
    got = _run(G, inp)
    _check_mix(got, _ref(inp))
    return got


# 2B = 64 (B = 32), 80 / 74 (direct kernel above 64 rows, K % 4 != 0), 128 (B == 64: one-launch backward), 192 (blocked),
# 256 (gram_q256; K % 32 != 0: its ragged-K form), 384 (128-row tiles; the four solves at n = 192 on the multi-CU solver)
@pytest.mark.parametrize("B,K", [(32, 512), (40, 258), (37, 260), (64, 512), (96, 256), (128, 256), (128, 256 + 36),
                                 (192, 256)],
                         ids=["b32", "b40_ragged", "b37_odd", "b64", "b96_blocked", "b128_q256", "b128_q256_ragged_k",
                              "b192_tiled"])
def test_mixed_loss_on_every_cost_rung(G, L, B, K):
    got = _check_shape(G, L, B, K)
    assert got[3] == bool(L.lib.kccot_sinkhorn_fused_eligible(B, 100))


@pytest.mark.parametrize("variant", ["direct", "gram_f32", "no_tiles", "apply_m256_0", "apply_one_launch_0"])
def test_mixed_loss_b64_with_the_ladder_stepped_down(G, L, variant):
    opts = {"direct": (), "gram_f32": (("gram_f32", 1), ("apply_f32", 1)),
            "no_tiles": (("cost_tiled", 0), ("cost_tile256", 0), ("cost_blocked", 0)),
            "apply_m256_0": (("apply_m256", 0),), "apply_one_launch_0": (("apply_one_launch", 0),)}[variant]
    _check_shape(G, L, 64, 512, opts=opts, flags=L.COST_FORCE_DIRECT if variant == "direct" else 0)


def test_mixed_loss_b128_on_the_128_row_tiles(G, L):
    """2B = 256 with cost_tile256 = 0: the 128-row tiles of cost_tiled.hip instead of gram_q256."""
    _check_shape(G, L, 128, 256, opts=(("cost_tile256", 0),))


def test_mixed_loss_b192_four_problem_solver_forms(G, L):
    """n = 192 > 128: the four solves on the multi-CU solver.  Without the per-XCD layout (sinkhorn_coop_xcd = 0, the
    agent-scope exchange) the result is the same bits (include/kccot.h); the streaming solver (sinkhorn_coop = 0) is
    another kernel and is held to the fp64 oracle."""
    inp = _rand_inputs(192, 256, seed=1)
    ref = _ref(inp)
    base = _run(G, inp)
    _check_mix(base, ref)
    with L.options(sinkhorn_coop_xcd=0):
        agent = _run(G, inp)
    assert base[0] == agent[0]
    for a, b in zip(base[2], agent[2]):
        assert torch.equal(a, b)
    for k in WRT:
        np.testing.assert_array_equal(base[1][k], agent[1][k], err_msg=k)
    with L.options(sinkhorn_coop=0):
        _check_mix(_run(G, inp), ref)


def test_mixed_video_gradient_on_256x256_tiles(G, L):
    """2B = 256 and K = 131072: 512 column tiles, so the stacked video gradient d[y; y'] runs on the 256 x 256 tiles of
    cost_bwd_q256.hip (apply_q256 = 1, the default) -- bit-identical to the 256 x 64 / 128 tiles (apply_q256 = 0) and
    within 1e-4 of max|grad| of the fp64 gradient.  sc is scaled by 512 / K to keep the costs of the decimated shapes
    (K = 131072 at sc = 1/15 would be a far sharper problem).  The fp64 reference is the oracle's causal term and Sinkhorn
    solve on cost matrices from an fp64 Gram product, and the closed form of d C / d y (the oracle's broadcast cost_xy
    would hold [B,B,K] in fp64)."""
    B, K = 128, 131072
    sc = cases.SC * 512 / K
    inp = _rand_inputs(B, K, T=4, J=4, seed=2)
    wrt = ["fake", "fake_p"]
    out = {}
    for mode in (1, 0):
        with L.options(apply_q256=mode):
            out[mode] = _run(G, inp, wrt, sc=sc)
    for k in wrt:
        np.testing.assert_array_equal(out[1][1][k], out[0][1][k], err_msg=k)
    d = {k: torch.from_numpy(v.reshape(v.shape[0], -1)).double() for k, v in inp.items()}

    def sqd(a, b):
        return ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.t()) * sc

    C = []
    for a, b, h, m, _ in mixed_cases.TERMS:
        c = (sqd(d[a], d[b]) + ot.causal_term(d[h].reshape(B, 4, 4), d[m].reshape(B, 4, 4), sc)).requires_grad_(True)
        C.append(c)
    w = [ot.sinkhorn_from_cost(c, 1.0, 100)[0] for c in C]
    ref_val = (w[0] + w[1]) - w[2] - w[3]
    dC1, dC2, _, dC4 = torch.autograd.grad(ref_val, C)
    x, y, x_p, y_p = d["real"], d["fake"], d["real_p"], d["fake_p"]
    # C1 = sc |x_i - y_j|^2, C2 = sc |x'_i - y'_j|^2, C4 = sc |y_i - y'_j|^2
    dy = 2 * sc * (dC1.sum(0)[:, None] * y - dC1.t() @ x + dC4.sum(1)[:, None] * y - dC4 @ y_p)
    dy_p = 2 * sc * (dC2.sum(0)[:, None] * y_p - dC2.t() @ x_p + dC4.sum(0)[:, None] * y_p - dC4.t() @ y)
    assert abs(out[1][0] - float(ref_val)) <= 1e-4 * max(abs(float(ref_val)), max(abs(float(v)) for v in w))
    for k, ref in (("fake", dy.numpy()), ("fake_p", dy_p.numpy())):
        np.testing.assert_allclose(out[1][1][k].reshape(B, K), ref, rtol=0, atol=1e-4 * np.abs(ref).max(), err_msg=k)


def test_mixed_loss_on_random_ragged_shapes(G):
    """20 seeded configurations in the style of test_gpu_parity.py::test_loss_and_gradients_on_random_ragged_shapes: B from
    1 to 70 (odd, prime, one sample, just above 64, not a multiple of 16), T = 1 (no causal term: the six feature
    gradients are exactly zero) to 6, J = 1 .. 5, K not a multiple of 4, sc in {1/15, 1, 0.01}, near and far regimes --
    against the fp64 oracle (loss at 1e-4 of max(|loss|, max |W_k|), gradients at the floor / 4 x the far-regime gap)."""
    rng = np.random.default_rng(20263)
    for trial in range(20):
        B = int(rng.choice([1, 2, 3, 5, 7, 11, 17, 23, 31, 33, 48, 63, 65, 70]))
        T, J = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        K = 4 * int(rng.integers(1, 40)) + int(rng.integers(1, 4))
        far = bool(rng.integers(0, 2))
        sc = float(rng.choice([cases.SC, 1.0, 0.01]))
        inp = _rand_inputs(B, K, T, J, seed=trial, far=far)
        tag = (trial, B, T, J, K, far, sc)
        got = _run(G, inp, sc=sc)
        ref = _ref(inp, sc=sc)
        if T == 1:
            assert all(np.abs(got[1][k]).max() == 0 for k in WRT[2:]), tag
        tol = max(2.5e-5, 4 * 2.5e-4 if far else 0.0) * 4
        try:
            _check_mix(got, ref, gtol=tol, loss_abs=2e-6)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (tag, e))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("part", ["features", "videos", "fake_p"])
def test_mixed_loss_partial_gradients(G, L, part, fused):
    """Discriminator step (videos detached: dF is NULL), generator step (every feature detached: every feature-gradient
    pointer NULL) and y' alone: the requested gradients match the fp64 ones; the loss node hands back None for the rest."""
    L.set_option("sinkhorn_fused", fused)
    wrt = {"features": WRT[2:], "videos": ["fake", "fake_p"], "fake_p": ["fake_p"]}[part]
    inp = _rand_inputs(48, 258, T=5, J=3, seed=7)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    for k in wrt:
        t[k].requires_grad_(True)
    loss = call(G, t)
    assert G.last_info["compute_mixed_sinkhorn_loss_fused_sweep"] == bool(fused)
    node = loss.grad_fn.apply(torch.ones((), device=DEV))          # (7 x None, d[y; y'], six feature gradients)
    assert all(x is None for x in node[:7])
    assert (node[7] is None) == (part == "features")
    feats = ["h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p"]
    for k, x in zip(feats, node[8:]):
        assert (x is None) == (k not in wrt), k
    grads = dict(zip(wrt, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in wrt]))))
    ref_val, ref_w, ref_C, ref_g = _ref(inp, wrt)
    got = (float(loss), grads, [G.last_info["compute_mixed_sinkhorn_loss" + s] for s in ("", "_costs", "_Cmix")], None)
    _check_mix(got, (ref_val, ref_w, ref_C, ref_g))
