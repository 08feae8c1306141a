"""The fused solve + reverse sweep (sinkhorn_fused_reg) away from its default window: 64 < n <= 128 (option
"sinkhorn_fused_max_n" = 128, the <16, 8> instances), the four-problem instances at every lanes-per-line setting
(<2,16>, <4,16>, <8,8>, <16,4>), and the LDS-capacity edge of kccot_sinkhorn_fused_eligible (the dual history fills
exactly 144 KB at n = 128, L = 143 and at n = 64, L = 287).

The fused launch and the history form (forward kernel + global dual history + sweep kernel) run the same arithmetic
instruction for instruction: at matched lanes per line, loss, costs, iteration counts, cost matrices and every gradient
are bit-identical.  Both are also held to the fp64 torch oracle (the compositions of the loss's own test file): cost
matrices 1e-5 of max|C|, loss 1e-4 of max(|loss|, max |W|), gradients 1e-4 of max|grad| (near inputs) or, for the sharp
problems at the LDS edge (C / eps spans ~250, the solves run to L), the far-regime rule of the random ragged-shape tests,
4 x (4 x 2.5e-4) (measured on the MI355X: <= 1.4e-3), or 16 x the oracle's own fp32 / fp64 gap of the case if larger."""
import numpy as np
import pytest
import torch

import bicausal_cases
import cases
import mixed_cases
from oracle import gan_utils_torch as ot

DEV = "cuda:0"
ONE_TERMS = (("real", "fake", "h_fake", "m_real"), ("real", "real", "h_real", "m_real"),
             ("fake", "fake", "h_fake", "m_fake"))
# name -> (wrt, last_info tag, key of the cost matrices)
LOSSES = {
    "one": (["fake", "h_fake", "h_real", "m_real", "m_fake"], "compute_sinkhorn_loss", "_C3"),
    "bicausal": (["fake", "h_fake", "h_real", "m_real", "m_fake"], "compute_bicausal_sinkhorn_loss", "_C3"),
    "mixed": (["fake", "fake_p", "h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p"],
              "compute_mixed_sinkhorn_loss", "_Cmix"),
}


@pytest.fixture(scope="module")
def G():
    from kccotgan_amd import gan_utils
    return gan_utils


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _reset_flags(L):
    defaults = {k: L.get_option(k) for k in L.option_names()}
    yield
    for k, v in defaults.items():
        L.set_option(k, v)


def _inputs(B, K, T=6, J=4, seed=0, far=False):
    """Every operand any of the three losses takes: videos [B,1,K] (fake = real + 0.05 noise, or uniform when far)."""
    rng = np.random.default_rng(4000 + B + seed)
    inp = {}
    for k, src in (("real", None), ("fake", "real"), ("real_p", None), ("fake_p", "real_p")):
        if src is None or far:
            inp[k] = rng.random((B, 1, K), dtype=np.float32)
        else:
            inp[k] = np.clip(inp[src] + np.float32(0.05) * rng.standard_normal((B, 1, K), dtype=np.float32), 0,
                             1).astype(np.float32)
    for k in ("h_fake", "h_real", "m_real", "m_fake", "h_real_p", "h_fake_p", "m_real_p"):
        inp[k] = rng.random((B, T, J), dtype=np.float32)
    return inp


def _call(G, name, t, sc, eps, Lit, honor):
    if name == "mixed":
        return G.compute_mixed_sinkhorn_loss(t["real"], t["fake"], t["real_p"], t["fake_p"], sc, eps, Lit, t["h_fake"],
                                             t["m_real"], t["h_real_p"], t["m_fake"], t["h_fake_p"], t["m_real_p"],
                                             honor_eps_l=honor)
    fn = G.compute_sinkhorn_loss if name == "one" else G.compute_bicausal_sinkhorn_loss
    return fn(t["real"], t["fake"], sc, eps, Lit, t["h_fake"], t["m_real"], t["h_real"], t["m_fake"], honor_eps_l=honor)


def _run(G, name, inp, sc=cases.SC, eps=1.0, Lit=100, honor=False):
    """(loss, nits, costs, C, {wrt: grad}, fused_sweep) of one GPU evaluation with every gradient of the loss."""
    wrt, tag, key = LOSSES[name]
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    for k in wrt:
        t[k].requires_grad_(True)
    loss = _call(G, name, t, sc, eps, Lit, honor)
    info = [G.last_info[tag + s].clone() for s in ("", "_costs", key)]
    fused = G.last_info[tag + "_fused_sweep"]
    G.raise_if_solver_aborted((tag,))
    grads = dict(zip(wrt, (x.cpu().numpy() for x in torch.autograd.grad(loss, [t[k] for k in wrt]))))
    return (loss.detach().cpu().numpy().reshape(1), *info, grads, fused)


def _oracle(name, inp, dtype, sc=cases.SC, eps=1.0, Lit=100):
    """(loss, [W], [C], {wrt: grad}) of the oracle composition in `dtype`."""
    wrt = LOSSES[name][0]
    d = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items()}
    for k in wrt:
        d[k].requires_grad_(True)
    if name == "one":
        C = [ot.modified_cost(d[a], d[b], d[h], d[m], sc, 16) for a, b, h, m in ONE_TERMS]
        wts = (2.0, -1.0, -1.0)
    elif name == "bicausal":
        C = [ot.bi_causal_modified_cost(d[a], d[b], d[hy], d[mx], d[hx], d[my], sc, 16)
             for _, a, b, hy, mx, hx, my in bicausal_cases.TERMS]
        wts = (2.0, -1.0, -1.0)
    else:
        C = [ot.modified_cost(d[a], d[b], d[h], d[m], sc, 16) for a, b, h, m, _ in mixed_cases.TERMS]
        wts = tuple(s for *_, s in mixed_cases.TERMS)
    w = [ot.sinkhorn_from_cost(c, eps, Lit)[0] for c in C]
    val = sum(s * x for s, x in zip(wts, w))
    grads = dict(zip(wrt, (x.double().numpy() for x in torch.autograd.grad(val, [d[k] for k in wrt]))))
    return float(val), [float(x) for x in w], [c.detach().double().numpy() for c in C], grads


def _same(a, b):
    """Bit-identical runs (_run tuples): loss, counts, costs, matrices, gradients."""
    assert a[0].view(np.int32) == b[0].view(np.int32), (a[0], b[0])
    for x, y, what in zip(a[1:4], b[1:4], ("nits", "costs", "C")):
        assert torch.equal(x, y), what
    for k in a[4]:
        np.testing.assert_array_equal(a[4][k], b[4][k], err_msg=k)


def _near_oracle(got, ref, gtol):
    loss, _, costs, C, grads, _ = got
    ref_val, ref_w, ref_C, ref_g = ref
    C, costs = C.cpu().numpy(), costs.cpu().numpy()
    for k in range(len(ref_w)):
        np.testing.assert_allclose(C[k], ref_C[k], rtol=0, atol=1e-5 * np.abs(ref_C[k]).max(), err_msg="C%d" % k)
        assert abs(costs[k] - ref_w[k]) <= 1e-4 * abs(ref_w[k]) + 1e-5 * np.abs(ref_C[k]).max(), (k, costs[k], ref_w[k])
    assert abs(float(loss[0]) - ref_val) <= 1e-4 * max(abs(ref_val), max(abs(x) for x in ref_w)), (float(loss[0]), ref_val)
    for k, b in ref_g.items():
        tol = gtol[k] if isinstance(gtol, dict) else gtol
        np.testing.assert_allclose(grads[k], b, rtol=0, atol=tol * np.abs(b).max(), err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 96, 128])
@pytest.mark.parametrize("name", ["one", "bicausal", "mixed"])
def test_fused_sweep_above_64_equals_the_history_form(G, L, name, n):
    """sinkhorn_fused_max_n = 128: the solves and the sweep of n = 65 .. 128 in one launch (sinkhorn_fused_reg<16, 8>,
    three or four problems) against sinkhorn_fused = 0 (8 lanes per line forward and backward above 64)."""
    inp = _inputs(n, 260, seed=1)
    L.set_option("sinkhorn_fused_max_n", 128)
    fused = _run(G, name, inp)
    L.set_option("sinkhorn_fused", 0)
    hist = _run(G, name, inp)
    assert fused[5] is True and hist[5] is False
    _same(fused, hist)
    _near_oracle(fused, _oracle(name, inp, torch.float64), 1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [4, 8, 16])
@pytest.mark.parametrize("n", [24, 48])
def test_mixed_fused_sweep_at_every_lanes_per_line(G, L, n, lanes):
    """Four problems on <2,16> (n = 24, any lanes option) and on <16,4> / <8,8> / <4,16> (n = 48 at 4 / 8 / 16 lanes per
    line): the fused launch equals the history form run at the same lanes per line, and the fp64 oracle."""
    inp = _inputs(n, 258, seed=2)
    L.set_option("sinkhorn_lanes_per_line", lanes)
    fused = _run(G, "mixed", inp)
    L.set_option("sinkhorn_fused", 0)
    hist = _run(G, "mixed", inp)
    assert fused[5] is True and hist[5] is False
    _same(fused, hist)
    _near_oracle(fused, _oracle("mixed", inp, torch.float64), 1e-4)


EDGES = [(128, 143), (64, 287)]     # the largest L whose dual history fits 144 KB: 2 (L + 1) NS 4 bytes, NS = 128 / 64


def test_fused_eligibility_at_the_lds_edge(L):
    with L.options(sinkhorn_fused_max_n=128):
        assert L.lib.kccot_sinkhorn_fused_eligible(128, 143) == 1 and L.lib.kccot_sinkhorn_fused_eligible(128, 144) == 0
        assert L.lib.kccot_sinkhorn_fused_eligible(65, 143) == 1 and L.lib.kccot_sinkhorn_fused_eligible(65, 144) == 0
    assert L.lib.kccot_sinkhorn_fused_eligible(128, 143) == 0          # default sinkhorn_fused_max_n = 64
    for lanes in (0, 4, 8, 16):                                         # NS = 64 at every lanes-per-line setting
        with L.options(sinkhorn_lanes_per_line=lanes):
            assert L.lib.kccot_sinkhorn_fused_eligible(64, 287) == 1 and L.lib.kccot_sinkhorn_fused_eligible(64, 288) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,Lit", EDGES, ids=["n128_L143", "n64_L287"])
@pytest.mark.parametrize("name", ["one", "bicausal", "mixed"])
def test_fused_sweep_at_the_lds_edge(G, L, name, n, Lit):
    """honor_eps_l at the largest eligible L: fused == history form == fp64 oracle; at L + 1 the loss falls back to the
    history form and still matches the oracle (and, where no solve reached L, the L result bit for bit).  Sharp far-regime
    problems (sc = 1, eps = 0.05), so the solves run far past Lmin = 100 and use the last rows of the history."""
    inp = _inputs(n, 66, T=4, J=3, seed=3, far=True)
    kw = dict(sc=1.0, eps=0.05)
    L.set_option("sinkhorn_fused_max_n", 128)
    L.set_option("sinkhorn_lanes_per_line", 8)       # n = 64: the history form's sweep at the fused kernel's 8 lanes
    fused = _run(G, name, inp, Lit=Lit, honor=True, **kw)
    with L.options(sinkhorn_fused=0):
        hist = _run(G, name, inp, Lit=Lit, honor=True, **kw)
    over = _run(G, name, inp, Lit=Lit + 1, honor=True, **kw)
    assert fused[5] is True and hist[5] is False and over[5] is False
    _same(fused, hist)
    nits = fused[1].cpu().numpy()
    assert nits.max() > 100
    if nits.max() < Lit:
        _same(fused, over)
    for got, Lx in ((fused, Lit), (over, Lit + 1)):
        ref = _oracle(name, inp, torch.float64, Lit=Lx, **kw)
        ref32 = _oracle(name, inp, torch.float32, Lit=Lx, **kw)[3]
        tol = {k: max(4e-3, 16 * float(np.abs(ref32[k] - b).max() / np.abs(b).max())) for k, b in ref[3].items()}
        _near_oracle(got, ref, tol)
