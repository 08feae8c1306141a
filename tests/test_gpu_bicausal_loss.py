"""GPU tests of compute_bicausal_sinkhorn_loss (2 W(x,y) - W(x,x) - W(y,y) with the bi-causal cost, an extension of the
reference): against the fixtures written by tests/golden/make_bicausal_golden.py (the reference's own
compute_sinkhorn(..., bi_causal=True) per term), fp64 torch autograd of the oracle composition, the public generic
pieces, the one-batch loss in a degenerate case, every rung of the cost ladder and both backward forms, graph replay.

Tolerances follow tests/test_gpu_mixed_loss.py: costs 5e-5 (fp32 fixture) / 1e-4 (fp64) relative, cost matrices 1e-5 of
max|C|, iteration counts identical, gradients max(2.5e-5, 4 x the oracle's own fp32 / fp64 gap of the case) of max|grad|.
The loss 2 W_xy - W_xx - W_yy cancels in the near regime, so its 1e-4 bound is taken relative to max(|loss|, max |W|)."""
import json
import os

import numpy as np
import pytest
import torch

import bicausal_cases
import cases
from oracle import gan_utils_torch as ot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
GRAD_GAP = json.load(open(os.path.join(GOLD, "grad_gap.json")))["gaps"]
WRT = ["fake", "h_fake", "h_real", "m_real", "m_fake"]
TAG = "compute_bicausal_sinkhorn_loss"
CASE_IDS = lambda c: bicausal_cases.case_name(*c)
SMALL = [c for c in bicausal_cases.CASES if c[0] != "cfg2"]


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


def load(case):
    shape, seed, regime = case[:3]
    g = np.load(os.path.join(GOLD, bicausal_cases.case_name(*case) + ".npz"))
    inp = cases.gen_inputs(shape, seed, regime)
    np.testing.assert_array_equal(cases.checksum(inp), g["checksum"])
    return g, inp, {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}


def call(G, t, case=None, **kw):
    eps, L = (case[3], case[4]) if case is not None else (0.8, 100)
    if case is not None and not bicausal_cases.default_eps_l(eps, L):
        kw["honor_eps_l"] = True
    return G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"], cases.SC, eps, L, t["h_fake"], t["m_real"], t["h_real"],
                                            t["m_fake"], **kw)


def oracle(d, eps=1.0, L=100, chunk=None, video=True, sc=cases.SC):
    """torch composition of the reference's compute_sinkhorn(..., bi_causal=True) over the three terms; returns
    (loss, {tag: W}, {tag: C})."""
    fl = ot.flatten_video if video else (lambda v: v)
    v = dict(d, real=fl(d["real"]), fake=fl(d["fake"]))
    w, C = {}, {}
    for tag, a, b, hy, mx, hx, my in bicausal_cases.TERMS:
        C[tag] = ot.bi_causal_modified_cost(v[a], v[b], v[hy], v[mx], v[hx], v[my], sc, chunk)
        w[tag] = ot.sinkhorn_from_cost(C[tag], eps, L)[0]
    return 2.0 * w["xy"] - w["xx"] - w["yy"], w, C


def loss_tol(ref_loss, ws):
    return 1e-4 * max(abs(float(ref_loss)), max(abs(float(x)) for x in ws))


def grad_tol(shape, seed, regime):
    gaps = GRAD_GAP.get(cases.case_name(shape, seed, regime), {})
    return max(2.5e-5, 4.0 * max(gaps.values(), default=0.0))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("case", bicausal_cases.CASES, ids=CASE_IDS)
def test_bicausal_loss_matches_reference_terms(G, L, case, fused):
    g, inp, t = load(case)
    L.set_option("sinkhorn_fused", fused)
    t["fake"].requires_grad_(True)                 # a gradient wanted: the fused solve + sweep where eligible
    loss = call(G, t, case)
    assert G.last_info[TAG + "_fused_sweep"] == bool(fused and L.lib.kccot_sinkhorn_fused_eligible(
        inp["real"].shape[0], case[4]))
    nits = G.last_info[TAG].cpu().numpy().tolist()
    assert nits == [int(g["nits_" + tag]) for tag in ("xy", "xx", "yy")]
    costs = G.last_info[TAG + "_costs"].cpu().numpy()
    C3 = G.last_info[TAG + "_C3"].cpu().numpy()
    for k, tag in enumerate(("xy", "xx", "yy")):
        ref, ref64 = float(g["w_" + tag]), float(g["w_%s_f64" % tag])
        assert abs(costs[k] - ref) <= 5e-5 * abs(ref) and abs(costs[k] - ref64) <= 1e-4 * abs(ref64), (tag, costs[k], ref)
        for sfx in ("", "_f64"):
            C = g["C_" + tag + sfx]
            np.testing.assert_allclose(C3[k], C, rtol=0, atol=1e-5 * np.abs(C).max(), err_msg="C_" + tag + sfx)
    for sfx in ("", "_f64"):
        ws = [g["w_%s%s" % (tag, sfx)] for tag in ("xy", "xx", "yy")]
        assert abs(float(loss.detach()) - float(g["loss" + sfx])) <= loss_tol(g["loss" + sfx], ws), (float(loss), sfx)
    G.raise_if_solver_aborted((TAG,))


def test_bicausal_loss_forward_only_and_eps_l_default(G, L):
    case = ("small", 0, "near", 1.0, 100)
    g, inp, t = load(case)
    a = call(G, t)                                                    # no gradient: history-free forward
    assert G.last_info[TAG + "_fused_sweep"] is False
    b = G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"], cases.SC, 0.1, 5, t["h_fake"], t["m_real"], t["h_real"],
                                         t["m_fake"])
    assert float(a) == float(b)                                       # eps / L ignored by default, as the one-batch loss
    c = call(G, t, honor_eps_l=True)                                  # eps = 0.8, L = 100
    assert float(c) != float(a)
    ws = [g["w_" + tag] for tag in ("xy", "xx", "yy")]
    assert abs(float(a) - float(g["loss"])) <= loss_tol(g["loss"], ws)


def _oracle_grads(inp, dtype, eps=1.0, L=100, chunk=None, video=True):
    d = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in WRT:
        d[k].requires_grad_(True)
    val, w, _ = oracle(d, eps, L, chunk, video)
    return val, w, dict(zip(WRT, (x.double().numpy() for x in torch.autograd.grad(val, [d[k] for k in WRT]))))


def _gpu_grads(G, t, **kw):
    for k in WRT:
        t[k] = t[k].detach().clone().requires_grad_(True)
    loss = G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"], cases.SC, 0.8, 100, t["h_fake"], t["m_real"],
                                            t["h_real"], t["m_fake"], **kw)
    return loss, dict(zip(WRT, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in WRT]))))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("case", SMALL, ids=CASE_IDS)
def test_bicausal_loss_gradients_match_fp64_autograd(G, L, case, fused):
    shape, seed, regime, eps, Lit = case
    g, inp, t = load(case)
    L.set_option("sinkhorn_fused", fused)
    ref_val, ref_w, ref = _oracle_grads(inp, torch.float64, eps, Lit)
    _, _, ref32 = _oracle_grads(inp, torch.float32, eps, Lit)
    for k in WRT:
        t[k].requires_grad_(True)
    loss = call(G, t, case)
    got = dict(zip(WRT, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in WRT]))))
    assert abs(float(loss) - float(ref_val)) <= loss_tol(ref_val, ref_w.values())
    for k in WRT:
        gap = float(np.abs(ref32[k] - ref[k]).max() / np.abs(ref[k]).max())
        tol = max(grad_tol(shape, seed, regime), 4.0 * gap)
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=tol * np.abs(ref[k]).max(), err_msg=k)


def test_composition_with_the_public_generic_pieces(G, L):
    """C3 equals bi_causal_modified_cost through the generic pairwise path; the loss equals 2 W_xy - W_xx - W_yy of three
    public compute_sinkhorn(bi_causal=True) calls."""
    g, inp, t = load(("deci64", 0, "near", 1.0, 100))
    loss = call(G, t)
    C3 = G.last_info[TAG + "_C3"].clone()
    w = {}
    for k, (tag, a, b, hy, mx, hx, my) in enumerate(bicausal_cases.TERMS):
        C = G.bi_causal_modified_cost(t[a], t[b], t[hy], t[mx], t[hx], t[my], cases.SC)
        torch.testing.assert_close(C3[k], C, rtol=0, atol=1e-6 * float(C.abs().max()))
        w[tag] = G.compute_sinkhorn(t[a], t[b], t[hy], t[mx], cases.SC, hx=t[hx], My=t[my], bi_causal=True)
    comp = 2 * w["xy"] - w["xx"] - w["yy"]
    assert abs(float(loss) - float(comp)) <= 1e-5 * max(abs(float(v)) for v in w.values()), (float(loss), float(comp))


@pytest.mark.parametrize("fused", [1, 0])
def test_degenerate_case_equals_the_one_batch_loss(G, L, fused):
    """h_real = 0 and m_fake constant in time: every causal term the bi-causal loss adds is exactly zero.  Loss, counts,
    dfake, dh_fake and dm_real equal the one-batch loss's; dh_real and dm_fake are twice the one-batch gradients (the xx /
    yy causal term counts twice)."""
    L.set_option("sinkhorn_fused", fused)
    g, inp, t = load(("deci64", 0, "near", 1.0, 100))
    t["h_real"] = torch.zeros_like(t["h_real"])
    t["m_fake"] = t["m_fake"][:, :1].expand_as(t["m_fake"]).contiguous()
    one_t = dict(t)
    for k in WRT:
        one_t[k] = t[k].clone().requires_grad_(True)
    one = G.compute_sinkhorn_loss(one_t["real"], one_t["fake"], cases.SC, 0.8, 100, one_t["h_fake"], one_t["m_real"],
                                  one_t["h_real"], one_t["m_fake"])
    one_nits = G.last_info["compute_sinkhorn_loss"].clone()
    one_C3 = G.last_info["compute_sinkhorn_loss_C3"].clone()
    d1 = dict(zip(WRT, torch.autograd.grad(one, [one_t[k] for k in WRT])))
    bc, d2 = _gpu_grads(G, t)
    assert torch.equal(G.last_info[TAG], one_nits)
    assert torch.equal(G.last_info[TAG + "_C3"], one_C3)
    assert float(bc) == float(one)
    d2 = {k: torch.from_numpy(v).to(DEV) for k, v in d2.items()}
    for k in ("fake", "h_fake", "m_real"):
        torch.testing.assert_close(d2[k], d1[k], rtol=0, atol=1e-6 * float(d1[k].abs().max()), msg=k)
    for k in ("h_real", "m_fake"):
        torch.testing.assert_close(d2[k], 2 * d1[k], rtol=0, atol=1e-6 * float(d1[k].abs().max()), msg=k)
    assert float(d1["h_real"].abs().max()) > 0 and float(d1["m_fake"].abs().max()) > 0


def _rand_inputs(B, K, T=8, J=8, seed=0):
    # videos as [B, 1, K]: the oracle's cost_xy sums the last two axes, the library flattens every trailing axis
    rng = np.random.default_rng(1000 + B + seed)
    real = rng.random((B, 1, K), dtype=np.float32)
    fake = np.clip(real + np.float32(0.05) * rng.standard_normal((B, 1, K), dtype=np.float32), 0, 1).astype(np.float32)
    inp = dict(real=real, fake=fake)
    for k in ("h_fake", "h_real", "m_real", "m_fake"):
        inp[k] = rng.random((B, T, J), dtype=np.float32)
    return inp


def _check_shape(G, L, B, K, opts=(), flags=0, tol=1e-4):
    for k, v in opts:
        L.set_option(k, v)
    G.cost_flags = flags
    inp = _rand_inputs(B, K)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    ref_val, ref_w, ref = _oracle_grads(inp, torch.float64, chunk=16, video=False)
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    _, _, refC = oracle(d, chunk=16, video=False)
    loss, got = _gpu_grads(G, t)
    G.raise_if_solver_aborted((TAG,))
    C3 = G.last_info[TAG + "_C3"].cpu().numpy()
    for k, tag in enumerate(("xy", "xx", "yy")):
        C = refC[tag].numpy()
        np.testing.assert_allclose(C3[k], C, rtol=0, atol=1e-5 * np.abs(C).max(), err_msg="C_" + tag)
    assert abs(float(loss) - float(ref_val)) <= loss_tol(ref_val, ref_w.values()), (float(loss), float(ref_val))
    for k in WRT:
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=tol * np.abs(ref[k]).max(), err_msg=k)


# every rung of the cost ladder and the backward paths above B = 64 (decimated K: >= 256 and a multiple of 4)
@pytest.mark.parametrize("B,K", [(128, 512), (256, 256), (384, 256), (192, 256), (40, 258)],
                         ids=["b128", "b256_multicu", "b384_tiled", "b192_blocked", "b40_ragged"])
def test_bicausal_loss_on_every_cost_rung(G, L, B, K):
    _check_shape(G, L, B, K)


@pytest.mark.parametrize("variant", ["direct", "gram_f32", "no_tiles"])
def test_bicausal_loss_b64_with_the_ladder_stepped_down(G, L, variant):
    opts = {"direct": (), "gram_f32": (("gram_f32", 1), ("apply_f32", 1)),
            "no_tiles": (("cost_tiled", 0), ("cost_tile256", 0), ("cost_blocked", 0))}[variant]
    _check_shape(G, L, 64, 512, opts=opts, flags=L.COST_FORCE_DIRECT if variant == "direct" else 0)


def test_fused_and_history_forms_agree_at_b64(G, L):
    inp = _rand_inputs(64, 1024, T=30, seed=3)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    out = {}
    for form, opts in (("fused", (("sinkhorn_fused", 1), ("apply_one_launch", 1))),
                       ("history", (("sinkhorn_fused", 0), ("apply_one_launch", 0)))):
        for k, v in opts:
            L.set_option(k, v)
        loss, grads = _gpu_grads(G, dict(t))
        out[form] = (float(loss), G.last_info[TAG].clone(), G.last_info[TAG + "_costs"].clone(),
                     G.last_info[TAG + "_C3"].clone(), grads, G.last_info[TAG + "_fused_sweep"])
    f, h = out["fused"], out["history"]
    assert f[5] is True and h[5] is False
    assert f[0] == h[0] and torch.equal(f[1], h[1]) and torch.equal(f[2], h[2]) and torch.equal(f[3], h[3])
    for k in WRT:
        np.testing.assert_allclose(f[4][k], h[4][k], rtol=0, atol=1e-5 * np.abs(h[4][k]).max(), err_msg=k)


def test_bicausal_loss_errors(G, L):
    g, inp, t = load(("tiny", 0, "near", 1.0, 100))
    r = t["real"].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError):
        G.compute_bicausal_sinkhorn_loss(r, t["fake"], cases.SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                         t["m_fake"])
    with pytest.raises(ValueError):
        G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"][:-1], cases.SC, 0.8, 100, t["h_fake"], t["m_real"],
                                         t["h_real"], t["m_fake"])
    with pytest.raises(ValueError):
        G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"], cases.SC, 0.8, 100, t["h_fake"][:, 1:], t["m_real"],
                                         t["h_real"], t["m_fake"])


@pytest.mark.parametrize("fused", [1, 0])
def test_bicausal_loss_graph_replay_equals_eager(G, L, fused):
    g, inp, t = load(("deci64", 0, "near", 1.0, 100))
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
                for k in ("fake", "h_real", "m_fake"):
                    t[k].copy_(torch.from_numpy(np.clip(inp[k] + np.float32(0.01) * rng.standard_normal(inp[k].shape,
                                                                                              dtype=np.float32), 0, 1)))
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)


def _check_against_oracle(G, inp, wrt, sc, gtol, loss_abs=0.0, tag=None):
    """The loss with gradients of `wrt` against the fp64 oracle: C3 at 1e-5 of max|C|, costs 1e-4 relative (+ 1e-5 of
    max|C|), loss per loss_tol (+ loss_abs), gradients gtol of max|grad| (exactly zero where the oracle's are)."""
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    for k in wrt:
        t[k].requires_grad_(True)
    loss = G.compute_bicausal_sinkhorn_loss(t["real"], t["fake"], sc, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                            t["m_fake"])
    G.raise_if_solver_aborted((TAG,))
    got = dict(zip(wrt, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in wrt], retain_graph=True))))
    d = {k: torch.from_numpy(v).double() for k, v in inp.items()}
    for k in wrt:
        d[k].requires_grad_(True)
    ref_val, ref_w, refC = oracle(d, chunk=16, video=False, sc=sc)
    ref = dict(zip(wrt, (x.numpy() for x in torch.autograd.grad(ref_val, [d[k] for k in wrt]))))
    C3 = G.last_info[TAG + "_C3"].cpu().numpy()
    costs = G.last_info[TAG + "_costs"].cpu().numpy()
    for k, name in enumerate(("xy", "xx", "yy")):
        C = refC[name].detach().numpy()
        np.testing.assert_allclose(C3[k], C, rtol=0, atol=1e-5 * np.abs(C).max(), err_msg=str((tag, "C_" + name)))
        w = float(ref_w[name])
        assert abs(costs[k] - w) <= 1e-4 * abs(w) + 1e-5 * np.abs(C).max(), (tag, name, costs[k], w)
    assert abs(float(loss) - float(ref_val)) <= loss_tol(ref_val, ref_w.values()) + loss_abs, (tag, float(loss),
                                                                                                 float(ref_val))
    for k in wrt:
        scale = np.abs(ref[k]).max()
        if scale == 0:
            assert np.abs(got[k]).max() == 0, (tag, k)
            continue
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=gtol * scale, err_msg=str((tag, k)))
    return loss


def test_bicausal_loss_on_random_ragged_shapes(G):
    """20 seeded configurations in the style of test_gpu_parity.py::test_loss_and_gradients_on_random_ragged_shapes: B from
    1 to 70, T = 1 (no causal term: the four feature gradients are exactly zero) to 6, J = 1 .. 5, K not a multiple of 4,
    sc in {1/15, 1, 0.01}, near and far regimes -- against the fp64 oracle (loss per loss_tol, gradients at the floor /
    4 x the far-regime gap)."""
    rng = np.random.default_rng(20264)
    for trial in range(20):
        B = int(rng.choice([1, 2, 3, 5, 7, 11, 17, 23, 31, 33, 48, 63, 65, 70]))
        T, J = int(rng.integers(1, 7)), int(rng.integers(1, 6))
        K = 4 * int(rng.integers(1, 40)) + int(rng.integers(1, 4))
        far = bool(rng.integers(0, 2))
        sc = float(rng.choice([cases.SC, 1.0, 0.01]))
        inp = _rand_inputs(B, K, T, J, seed=trial)
        if far:
            inp["fake"] = np.random.default_rng(trial).random(inp["real"].shape, dtype=np.float32)
        tol = max(2.5e-5, 4 * 2.5e-4 if far else 0.0) * 4
        _check_against_oracle(G, inp, WRT, sc, tol, loss_abs=2e-6, tag=(trial, B, T, J, K, far, sc))


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("part", ["features", "videos"])
def test_bicausal_loss_partial_gradients(G, L, part, fused):
    """Discriminator step (fake detached: dfake is NULL) and generator step (every feature detached: every feature-gradient
    pointer NULL): the requested gradients match the fp64 ones; the loss node hands back None for the rest."""
    L.set_option("sinkhorn_fused", fused)
    wrt = WRT[1:] if part == "features" else ["fake"]
    inp = _rand_inputs(48, 258, T=5, J=3, seed=7)
    loss = _check_against_oracle(G, inp, wrt, cases.SC, 1e-4)
    assert G.last_info[TAG + "_fused_sweep"] == bool(fused)
    node = loss.grad_fn.apply(torch.ones((), device=DEV))     # (7 x None, dfake, dh_fake, dh_real, dm_real, dm_fake)
    assert all(x is None for x in node[:7])
    for k, x in zip(["fake", "h_fake", "h_real", "m_real", "m_fake"], node[7:]):
        assert (x is None) == (k not in wrt), k
