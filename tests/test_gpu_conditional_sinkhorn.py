"""The kernel-conditional Sinkhorn loss on the device (include/kccot_conditional.h, gan_utils.kernel_conditional_weights /
compute_conditional_sinkhorn_loss, KCCOTTrainer(conditional_bandwidth=...)) held to the float64 yardsticks of
tests/test_conditional_sinkhorn_cpu.py.

Tolerance (measured, not invented): in the same test the composition the library offered before -- the weighted entry points
of include/kccot_weighted.h on a [3Q,n,n] expanded copy of C3 with gcost = gloss omega_q {2,-1,-1}, the Q gradients summed in
float64 on the host; compute_weighted_sinkhorn_loss at the loss level; torch.softmax in fp32 for the weights -- is measured
against float64 on the same inputs.  That relative error is the yardstick, and a result of the new path must satisfy
    |got - ref| <= 4 max(yardstick, 2^-24) max|ref|
per quantity.  The factor and the floor are those of tests/test_gpu_weighted_sinkhorn.py, for the same reason: fp32 summation
order differs between otherwise equal computations.  Every test prints its figures before it asserts (-s).

Every buffer handed to the C ABI lies between NaN-filled guard zones that are verified after each call, workspaces are exactly
as long as the query functions say, and rejected calls must leave every output untouched.
"""
import functools
import math

import numpy as np
import pytest
import torch

import test_conditional_sinkhorn_cpu as CC
import test_gpu_weighted_sinkhorn as GW
import test_weighted_sinkhorn_cpu as W
from test_gpu_weighted_sinkhorn import Buf, call, rel_err, same_bits, within, workspace
from test_weighted_sinkhorn_cpu import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
I32 = torch.int32
SIZES = (5, 64, 67, 128, 130)
EPS_L = [(1.0, 100), (0.8, 7)]
QMAX = 7
GLOSS = (1.0, -0.5)


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


# ---------------------------------------------------------------- inputs and float64 references, computed once
@functools.lru_cache(maxsize=None)
def problem(n, Q=QMAX):
    """C3 [3,n,n] float32 (small_cost), Q weight rows float32 (random_weights), non-uniform query weights [Q] float32."""
    C3 = torch.stack([W.small_cost(n, 100 * n + k) for k in range(3)])
    w = torch.stack([W.random_weights(n, 3000 + 10 * n + q) for q in range(Q)]).float()
    omega = W.random_weights(Q, 77 + Q).float()
    return C3, w, omega


@functools.lru_cache(maxsize=None)
def reference(n, eps, Lit):
    """float64, for the QMAX queries of problem(n) on the float32 inputs the device reads: costs [QMAX,3], counts, and
    dcost[q,k] / dC3[k] as [QMAX,3,n,n].  Any (Q, omega, gloss) is a linear combination of these."""
    C3, w, _ = problem(n)
    C64 = C3.double().requires_grad_(True)
    costs, nits = CC.conditional_costs(C64, w.double(), eps, Lit)
    grads = torch.zeros(QMAX, 3, n, n, dtype=F64)
    for q in range(QMAX):
        for k in range(3):
            (g,) = torch.autograd.grad(costs[q][k], C64, retain_graph=True)
            assert float(g[[j for j in range(3) if j != k]].abs().max()) == 0.0
            grads[q, k] = g[k]
    return torch.tensor([[float(c.detach()) for c in row] for row in costs], dtype=F64), nits, grads


def combine64(costs, grads, omega, Q, gloss):
    """float64 loss and dC3 [3,n,n] from per-problem float64 (or float32) costs [Q,3] and gradients [Q,3,n,n]."""
    om = CC.query_weights(omega, Q)
    coef = torch.tensor(CC.COEF, dtype=F64)
    loss = (om[:, None] * coef[None, :] * costs[:Q].double()).sum()
    dC3 = gloss * (om[:, None, None, None] * coef[None, :, None, None] * grads[:Q].double()).sum(0)
    return loss, dC3


# ---------------------------------------------------------------- the new entry points through the C ABI, guarded
def cond_solve(L, C3, w, omega, eps, Lit, gloss=(1.0,), hist=True, bwd=True):
    """cost [Q,3], nits [2,Q,3], loss, [dC3 per gloss] of kccot_sinkhorn_conditional_fwd_f32 / _bwd_f32."""
    Q, n = w.shape
    Lh = max(Lit, 1)
    bufs = {"C3": Buf(C3.shape, C3), "w": Buf(w.shape, w), "u": Buf((Q, 3, Lh, n)), "v": Buf((Q, 3, Lh, n)),
            "cost": Buf((Q, 3)), "nits": Buf((2, Q, 3), dtype=I32), "loss": Buf((1,)), "dC3": Buf(C3.shape), "g": Buf((1,))}
    if omega is not None:
        bufs["omega"] = Buf((Q,), omega)
    op = bufs["omega"].ptr() if omega is not None else None
    ws, wsb = workspace(L.lib.kccot_sinkhorn_conditional_workspace_bytes(Q, n))
    assert wsb > 0
    bufs["ws"] = ws
    up, vp = (bufs["u"].ptr(), bufs["v"].ptr()) if hist else (None, None)
    call(L, "kccot_sinkhorn_conditional_fwd_f32", bufs["C3"].ptr(), bufs["w"].ptr(), op, Q, n, eps, Lit, W.LMIN, W.THRESH, up, vp,
         bufs["cost"].ptr(), bufs["nits"].ptr(), bufs["loss"].ptr(), ws.ptr(), wsb, None)
    dCs = []
    if bwd:
        for g in gloss:
            bufs["g"].t.fill_(g)
            call(L, "kccot_sinkhorn_conditional_bwd_f32", bufs["g"].ptr(), bufs["C3"].ptr(), bufs["w"].ptr(), op, bufs["u"].ptr(),
                 bufs["v"].ptr(), bufs["nits"].ptr(), Q, n, eps, Lh, bufs["dC3"].ptr(), ws.ptr(), wsb, None)
            dCs.append(bufs["dC3"].t.clone())
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d Q=%d)" % (k, n, Q)
    if not hist:
        assert bufs["u"].untouched() and bufs["v"].untouched()
    return bufs["cost"].t.clone(), bufs["nits"].t.clone(), bufs["loss"].t.clone(), dCs


def composition(L, C3, w, omega, eps, Lit, gloss):
    """What the library offered before: the weighted entry points on the [3Q,n,n] expanded copy, gcost = gloss omega_q {2,-1,-1},
    loss and the sum of the Q gradients in float64 on the host.  Returns costs [Q,3] (fp32), loss, dC3 (float64)."""
    Q, n = w.shape
    om = CC.query_weights(omega, Q)
    gc = (gloss * om[:, None] * torch.tensor(CC.COEF, dtype=F64)[None, :]).float().reshape(-1)
    Cx = C3.repeat(Q, 1, 1).contiguous()
    wx = w.repeat_interleave(3, dim=0).contiguous()
    cost, _, dC = GW.solve(L, Cx, wx, wx, eps, Lit, gcost=tuple(gc.tolist()))
    cost, dC = cost.cpu().view(Q, 3), dC.cpu().view(Q, 3, n, n)
    coef = torch.tensor(CC.COEF, dtype=F64)
    loss = (om[:, None] * coef[None, :] * cost.double()).sum()
    return cost, loss, dC.double().sum(0)


# ================================================================ 1. shared-cost indexing is exact
@pytest.mark.parametrize("eps,Lit", EPS_L)
@pytest.mark.parametrize("n", SIZES)
def test_shared_cost_indexing_is_bit_exact(L, n, eps, Lit):
    C3, w, _ = problem(n)
    Q = 3
    cost, nits, _, _ = cond_solve(L, C3, w[:Q].contiguous(), None, eps, Lit, bwd=False)
    for q in range(Q):
        w3 = w[q].expand(3, n).contiguous()
        c, k, _ = GW.solve(L, C3, w3, w3, eps, Lit, bwd=False)
        assert same_bits(cost[q], c), (n, q, cost[q], c)
        assert nits[0, q].tolist() == k[:3].tolist() and nits[1, q].tolist() == k[3:].tolist()
    assert len({tuple(cost[q].tolist()) for q in range(Q)}) == Q      # three different weight rows, three different answers


def test_shared_cost_indexing_with_more_workgroups_than_cus(L):
    n, Q, eps, Lit = 5, 90, 1.0, 100                                  # 270 workgroups
    C3, w, _ = problem(n, Q)
    cost, nits, _, _ = cond_solve(L, C3, w, None, eps, Lit, bwd=False)
    for q in range(Q):
        w3 = w[q].expand(3, n).contiguous()
        c, k, _ = GW.solve(L, C3, w3, w3, eps, Lit, bwd=False)
        assert same_bits(cost[q], c), (q, cost[q], c)
        assert nits[0, q].tolist() == k[:3].tolist() and nits[1, q].tolist() == k[3:].tolist()


# ================================================================ 2. float64 parity, the composition as the yardstick
@pytest.mark.parametrize("Q", [1, 3, 7])
@pytest.mark.parametrize("eps,Lit", EPS_L)
@pytest.mark.parametrize("n", SIZES)
def test_conditional_solver_against_fp64(L, n, eps, Lit, Q):
    C3, w, omega = problem(n)
    w = w[:Q].contiguous()
    ref_cost, ref_nits, ref_grads = reference(n, eps, Lit)
    worst = 0.0
    for om in (None, (omega[:Q] / omega[:Q].sum()).contiguous()):
        tag = "n=%d eps=%g L=%d Q=%d omega=%s" % (n, eps, Lit, Q, "1/Q" if om is None else "given")
        cost, nits, loss, dCs = cond_solve(L, C3, w, om, eps, Lit, gloss=GLOSS)
        assert nits[0].tolist() == [r for r in ref_nits[:Q]] == [[Lit] * 3] * Q
        for gi, gl in enumerate(GLOSS):
            y_cost, y_loss, y_dC = composition(L, C3, w, om, eps, Lit, gl)
            ref_loss, ref_dC = combine64(ref_cost, ref_grads, om, Q, gl)
            if gi == 0:
                worst = max(worst, within(tag + " loss", loss.cpu().reshape(()), ref_loss, rel_err(y_loss, ref_loss)))
                worst = max(worst, within(tag + " costs", cost.cpu(), ref_cost[:Q], rel_err(y_cost, ref_cost[:Q])))
                assert same_bits(cost.cpu(), y_cost)              # the same kernel on the same numbers
            worst = max(worst, within(tag + " dC3 gloss=%g" % gl, dCs[gi].cpu(), ref_dC, rel_err(y_dC, ref_dC)))
    print("WORST n=%d: %.2f" % (n, worst))


# ================================================================ 3. loss level and autograd
LOSS_CASES = [((6, 4, 8, 8, 1, 3), 6), ((64, 5, 8, 8, 1, 4), 64), ((130, 3, 4, 4, 1, 2), 5)]     # (B, T, H, W, C, J), Q
LOSS_EPS, LOSS_L = 0.8, 30        # L < Lmin = 100: every solve runs its 30 iterations; the float64 autograd reference stays quick
FEATS = ("h_fake", "m_real", "h_real", "m_fake")
NAMES = ("loss", "dfake", "dh_fake", "dm_real", "dh_real", "dm_fake")


@functools.lru_cache(maxsize=None)
def loss_inputs(shape, Q):
    B, T, H, Wd, Cc, J = shape
    rng = np.random.default_rng(11 + B)
    t = {"real": rng.random((B, H, T, Wd, Cc), dtype=np.float32), "fake": rng.random((B, H, T, Wd, Cc), dtype=np.float32)}
    t.update({k: rng.random((B, T, J), dtype=np.float32) for k in FEATS})
    t = {k: torch.from_numpy(v) for k, v in t.items()}
    t["w"] = torch.stack([W.random_weights(B, 500 + 7 * B + q) for q in range(Q)]).float()
    return t


@functools.lru_cache(maxsize=None)
def loss_reference(shape, Q, conditional):
    """float64 (loss, dfake, dh_fake, dm_real, dh_real, dm_fake): the conditional loss with omega = 1/Q, or (the yardstick's
    reference) the weighted loss with a = b = w[0]."""
    t = loss_inputs(shape, Q)
    B = shape[0]
    d = {k: t[k].double() for k in ("real", "fake") + FEATS}
    leaves = [d[k].requires_grad_(True) for k in ("fake",) + FEATS]
    x, y = d["real"].reshape(B, 1, -1), d["fake"].reshape(B, 1, -1)
    C3 = torch.stack([W.ot.modified_cost(x, y, d["h_fake"], d["m_real"], W.cases.SC),
                      W.ot.modified_cost(x, x, d["h_real"], d["m_real"], W.cases.SC),
                      W.ot.modified_cost(y, y, d["h_fake"], d["m_fake"], W.cases.SC)])
    w = t["w"].double()
    loss, _, nits = CC.conditional_loss_from_costs(C3, w if conditional else w[:1], None, LOSS_EPS, LOSS_L)
    assert all(k == [LOSS_L] * 3 for k in nits)
    return (loss.detach(),) + torch.autograd.grad(loss, leaves)


def run_loss(shape, Q, weights=None, query_weights=None, weighted_row=None):
    """(loss, dfake, four feature gradients) of compute_conditional_sinkhorn_loss, or (weighted_row given) of
    compute_weighted_sinkhorn_loss with w_real = w_fake = that vector."""
    from kccotgan_amd import gan_utils as g
    t = loss_inputs(shape, Q)
    real = t["real"].to(DEV)
    leaves = [t[k].to(DEV).requires_grad_(True) for k in ("fake",) + FEATS]
    fake, hf, mr, hr, mf = leaves
    if weighted_row is not None:
        wv = weighted_row.to(DEV)
        loss = g.compute_weighted_sinkhorn_loss(real, fake, W.cases.SC, LOSS_EPS, LOSS_L, hf, mr, hr, mf, wv, wv, normalize=False)
    else:
        qw = None if query_weights is None else query_weights.to(DEV)
        loss = g.compute_conditional_sinkhorn_loss(real, fake, W.cases.SC, LOSS_EPS, LOSS_L, hf, mr, hr, mf, weights.to(DEV), qw)
    grads = torch.autograd.grad(loss, leaves)
    torch.cuda.synchronize()
    return (loss.detach(),) + grads


@pytest.mark.parametrize("shape,Q", LOSS_CASES)
def test_loss_and_autograd_against_fp64(shape, Q):
    from kccotgan_amd import gan_utils as g
    t = loss_inputs(shape, Q)
    B = shape[0]
    ref_c, ref_w = loss_reference(shape, Q, True), loss_reference(shape, Q, False)
    got_w = run_loss(shape, Q, weighted_row=t["w"][0])
    got_c = run_loss(shape, Q, weights=t["w"])
    tag = "compute_conditional_sinkhorn_loss"
    info = g.last_info
    assert tuple(info[tag].shape) == (Q, 3) and info[tag].tolist() == [[LOSS_L] * 3] * Q
    assert tuple(info[tag + "_executed"].shape) == (Q, 3) and tuple(info[tag + "_costs"].shape) == (Q, 3)
    assert tuple(info[tag + "_C3"].shape) == (3, B, B) and info[tag + "_fused_sweep"] is False
    assert info[tag + "_path"] == ("register" if B <= 128 else "streaming")
    g.raise_if_solver_aborted((tag,))                                  # clean weights: nothing to report
    worst = 0.0
    for k, gc, rc, gw, rw in zip(NAMES, got_c, ref_c, got_w, ref_w):
        worst = max(worst, within("%s Q=%d %s" % (shape, Q, k), gc, rc.reshape(gc.shape), rel_err(gw, rw.reshape(gw.shape))))
    print("WORST loss %s Q=%d: %.2f" % (shape, Q, worst))


@pytest.mark.parametrize("shape,Q", [LOSS_CASES[0], LOSS_CASES[2]])
def test_equal_rows_give_the_weighted_loss_costs_bit_for_bit(shape, Q):
    from kccotgan_amd import gan_utils as g
    t = loss_inputs(shape, Q)
    wv = t["w"][1]
    run_loss(shape, Q, weighted_row=wv)
    want = g.last_info["compute_weighted_sinkhorn_loss_costs"].clone()
    got = run_loss(shape, Q, weights=wv.expand(Q, -1).contiguous())
    costs = g.last_info["compute_conditional_sinkhorn_loss_costs"]
    for q in range(Q):
        assert same_bits(costs[q], want), (q, costs[q], want)
    assert bool(torch.isfinite(got[0]))


def test_forward_and_backward_replay_from_a_graph_bit_for_bit():
    """The entry points allocate nothing and never synchronise: loss and gradients captured once replay to the eager bits."""
    from kccotgan_amd import gan_utils as g
    shape, Q = LOSS_CASES[0]
    t = loss_inputs(shape, Q)
    eager = run_loss(shape, Q, weights=t["w"])
    real, w = t["real"].to(DEV), t["w"].to(DEV)
    leaves = [t[k].to(DEV).requires_grad_(True) for k in ("fake",) + FEATS]
    fake, hf, mr, hr, mf = leaves

    def step():
        loss = g.compute_conditional_sinkhorn_loss(real, fake, W.cases.SC, LOSS_EPS, LOSS_L, hf, mr, hr, mf, w)
        return (loss,) + torch.autograd.grad(loss, leaves)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for k, a, b in zip(NAMES, out, eager):
        assert same_bits(a.detach().reshape(-1), b.reshape(-1)), k


def test_kernel_conditional_weights_wrapper_and_queries():
    from kccotgan_amd import gan_utils as g
    rng = np.random.default_rng(5)
    ctx = torch.from_numpy(rng.random((9, 4, 2, 4, 1), dtype=np.float32)).to(DEV)
    full = g.kernel_conditional_weights(ctx, 0.9)
    assert tuple(full.shape) == (9, 9) and full.dtype == F32
    idx = torch.tensor([7, 0, 3], device=DEV)
    part = g.kernel_conditional_weights(ctx, 0.9, queries=idx)
    D = torch.cdist(ctx.reshape(9, -1).double().cpu(), ctx.reshape(9, -1).double().cpu()) ** 2
    ref = CC.conditional_weights(D, 0.9)
    # the distances come from the library's fp32 cost kernel: a K = 32-term sum, |dD| <= 32 * 2^-24 max D ~ 1.5e-5, so a logit
    # is off by at most 1.5e-5 / (2 * 0.81) ~ 1e-5 and a weight (a ratio of two exponentials) by 2e-5 relative; twice that
    tol = 4e-5 * float(ref.max())
    assert float((full.double().cpu() - ref).abs().max()) <= tol
    assert float((part.double().cpu() - ref[idx.cpu()]).abs().max()) <= tol
    assert bool((full.argmax(1).cpu() == torch.arange(9)).all())     # a sample's own context weighs most


# ================================================================ 4. the weights kernel
def weights_abi(L, D, bw):
    Q, n = D.shape
    Db, out = Buf(D.shape, D), Buf((Q, n))
    call(L, "kccot_conditional_weights_f32", Db.ptr(), Q, n, bw, out.ptr(), None)
    assert Db.guards_intact() and out.guards_intact()
    return out.t.clone()


@functools.lru_cache(maxsize=None)
def distances(Q, n):
    g = torch.Generator().manual_seed(1000 * Q + n)
    c = torch.rand(n, 12, generator=g, dtype=F64)
    return (torch.cdist(c[:Q], c, compute_mode="donot_use_mm_for_euclid_dist") ** 2).float()


@pytest.mark.parametrize("Q,n", [(1, 1), (3, 5), (64, 64), (5, 67), (2, 1024)])
def test_weights_kernel_against_fp64(L, Q, n):
    D = distances(Q, n)
    dmax = max(float(D.max()), 1e-3)
    for lmax in (50.0, 5.0, 0.5):                      # bandwidths with max|l| = lmax <= 50: peaked, moderate, nearly flat
        bw = float(np.float32(math.sqrt(dmax / (2.0 * lmax)) * (1.0 + 1e-6)))
        assert float(D.max()) / (2.0 * bw * bw) <= 50.0
        ref = CC.conditional_weights(D, bw)
        logits = (-D.to(DEV) / (2.0 * bw * bw))
        yard = rel_err(torch.softmax(logits, dim=1), ref)
        got = weights_abi(L, D, bw)
        within("weights Q=%d n=%d max|l|=%g" % (Q, n, lmax), got, ref, yard)
        assert bool((got > 0).all()) and bool(torch.isfinite(got).all())
        dev = float((got.double().sum(1) - 1.0).abs().max())
        print("    max |row sum - 1| = %.3e (bound 2^-22 = %.3e)" % (dev, 2.0 ** -22))
        assert dev <= 2.0 ** -22
    uni = weights_abi(L, D, 1e30)
    want = np.float32(1.0) / np.float32(n)
    assert want == np.float32(1.0 / n)
    assert bool((uni.cpu() == float(want)).all())


def test_a_peaked_kernel_hits_the_floor_exactly_and_the_loss_stays_finite(L):
    n, Q = 5, 3
    D = distances(Q, n)
    w = weights_abi(L, D, 1e-3).cpu()
    off = torch.ones(Q, n, dtype=torch.bool)
    off[torch.arange(Q), torch.arange(Q)] = False
    assert bool((w[off] == 2.0 ** -100).all()) and bool((w[~off] == 1.0).all())
    C3, _, _ = problem(n)
    cost, nits, loss, dCs = cond_solve(L, C3, w.contiguous(), None, 1.0, 100, gloss=(1.0,))
    assert bool(torch.isfinite(cost).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dCs[0]).all())
    assert bool((nits[0] > 0).all())


# ================================================================ 5. poisoning is per query
@pytest.mark.parametrize("bad", [0.0, float("nan")])
def test_a_bad_weight_poisons_its_query_only(L, bad):
    n, Q = 64, 3
    C3, w, _ = problem(n)
    w = w[:Q].contiguous()
    good = cond_solve(L, C3, w, None, 1.0, 7)
    w2 = w.clone()
    w2[1, n // 3] = bad
    cost, nits, loss, dCs = cond_solve(L, C3, w2, None, 1.0, 7)
    assert bool(torch.isnan(cost[1]).all()) and nits[0, 1].tolist() == [-1] * 3
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dCs[0]).all())
    for q in (0, 2):
        assert same_bits(cost[q], good[0][q]) and nits[0, q].tolist() == [7] * 3
        assert nits[1, q].tolist() == good[1][1, q].tolist()


@pytest.mark.parametrize("bad", [0.0, float("nan")])
def test_raise_if_solver_aborted_reports_a_bad_weight(L, bad):
    from kccotgan_amd import gan_utils as g
    shape, Q = LOSS_CASES[0]
    t = loss_inputs(shape, Q)
    w = t["w"].clone()
    w[2, 1] = bad
    got = run_loss(shape, Q, weights=w)
    assert not bool(torch.isfinite(got[0])) and not bool(torch.isfinite(got[1]).any())
    counts = g.last_info["compute_conditional_sinkhorn_loss"]
    assert counts[2].tolist() == [-1] * 3 and bool((counts[[0, 1, 3, 4, 5]] == LOSS_L).all())
    with pytest.raises(L.KccotError, match="weight"):
        g.raise_if_solver_aborted(("compute_conditional_sinkhorn_loss",))
    run_loss(shape, Q, weights=t["w"])
    g.raise_if_solver_aborted(("compute_conditional_sinkhorn_loss",))


# ================================================================ 6. ABI hygiene
@pytest.mark.parametrize("n", [64, 130])
def test_null_histories_give_the_same_costs(L, n):
    C3, w, omega = problem(n)
    w, om = w[:3].contiguous(), omega[:3].contiguous()
    a = cond_solve(L, C3, w, om, 0.8, 7, bwd=False)
    b = cond_solve(L, C3, w, om, 0.8, 7, hist=False, bwd=False)
    assert same_bits(a[0], b[0]) and torch.equal(a[1], b[1]) and same_bits(a[2], b[2])


def test_rejected_calls_leave_every_output_untouched(L):
    EINVAL, EWORKSPACE, EUNSUPPORTED = L.EINVAL, L.EWORKSPACE, L.EUNSUPPORTED
    for n in (64, 130):
        C3, w, omega = problem(n)
        Q, Lit = 3, 7
        w = w[:Q].contiguous()
        Cb, wb, ob, gb = Buf(C3.shape, C3), Buf(w.shape, w), Buf((Q,), omega[:Q]), Buf((1,), torch.ones(1))
        outs = {k: Buf(s) for k, s in (("u", (Q, 3, Lit, n)), ("v", (Q, 3, Lit, n)), ("cost", (Q, 3)), ("nits", (2, Q, 3)),
                                       ("loss", (1,)), ("dC3", C3.shape))}
        need = L.lib.kccot_sinkhorn_conditional_workspace_bytes(Q, n)
        ws, wsb = workspace(need)

        def fwd(C_=Cb.ptr(), w_=wb.ptr(), Q_=Q, n_=n, eps_=1.0, L_=Lit, u_=outs["u"].ptr(), v_=outs["v"].ptr(),
                cost_=outs["cost"].ptr(), wsb_=wsb, want=EINVAL):
            call(L, "kccot_sinkhorn_conditional_fwd_f32", C_, w_, ob.ptr(), Q_, n_, eps_, L_, W.LMIN, W.THRESH, u_, v_, cost_,
                 outs["nits"].ptr(), outs["loss"].ptr(), ws.ptr(), wsb_, None, want=want)

        def bwd(C_=Cb.ptr(), w_=wb.ptr(), Q_=Q, n_=n, eps_=1.0, L_=Lit, u_=outs["u"].ptr(), v_=outs["v"].ptr(), wsb_=wsb,
                g_=gb.ptr(), want=EINVAL):
            call(L, "kccot_sinkhorn_conditional_bwd_f32", g_, C_, w_, ob.ptr(), u_, v_, outs["nits"].ptr(), Q_, n_, eps_, L_,
                 outs["dC3"].ptr(), ws.ptr(), wsb_, None, want=want)

        for f in (fwd, bwd):
            f(C_=None)
            f(w_=None)
            f(Q_=0)
            f(Q_=-2)
            f(n_=0)
            f(eps_=0.0)
            f(eps_=-1.0)
            f(L_=-1)
            f(n_=1025, want=EUNSUPPORTED)
            f(wsb_=need - 4, want=EWORKSPACE)
        fwd(u_=None)                       # histories not given together
        fwd(v_=None)
        fwd(cost_=None)
        bwd(u_=None)
        bwd(g_=None)
        assert all(o.untouched() for o in outs.values()) and ws.untouched()
    # the weights kernel
    D = distances(3, 5)
    Db, out = Buf(D.shape, D), Buf(D.shape)
    for args, want in (((None, 3, 5, 1.0, out.ptr()), EINVAL), ((Db.ptr(), 3, 5, 1.0, None), EINVAL),
                       ((Db.ptr(), 0, 5, 1.0, out.ptr()), EINVAL), ((Db.ptr(), 3, 0, 1.0, out.ptr()), EINVAL),
                       ((Db.ptr(), 3, 5, 0.0, out.ptr()), EINVAL), ((Db.ptr(), 3, 5, -1.0, out.ptr()), EINVAL),
                       ((Db.ptr(), 3, 5, float("nan"), out.ptr()), EINVAL), ((Db.ptr(), 3, 1025, 1.0, out.ptr()), EUNSUPPORTED)):
        call(L, "kccot_conditional_weights_f32", *args, None, want=want)
    assert out.untouched()
    # the loss entry points
    shape, Q = LOSS_CASES[0]
    t = loss_inputs(shape, Q)
    B, T, H, Wd, Cc, J = shape
    K = T * H * Wd * Cc
    ins = {k: Buf((B, K) if k in ("real", "fake") else t[k].shape, t[k].reshape(B, -1) if k in ("real", "fake") else t[k])
           for k in ("real", "fake") + FEATS}
    wq, g1 = Buf((Q, B), t["w"]), Buf((1,), torch.ones(1))
    outs = {k: Buf(s) for k, s in (("C3", (3, B, B)), ("u", (Q, 3, 7, B)), ("v", (Q, 3, 7, B)), ("cost", (Q, 3)), ("nits", (2, Q, 3)),
                                   ("loss", (1,)), ("dfake", (B, K)), ("dh_fake", (B, T, J)), ("dh_real", (B, T, J)),
                                   ("dm_real", (B, T, J)), ("dm_fake", (B, T, J)))}
    need = L.lib.kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, Q)
    ws, wsb = workspace(need)
    feats = [ins[k].ptr() for k in ("h_fake", "h_real", "m_real", "m_fake")]

    def lfwd(w_=wq.ptr(), B_=B, Q_=Q, eps_=1.0, u_=outs["u"].ptr(), wsb_=wsb, want=EINVAL):
        call(L, "kccot_conditional_sinkhorn_loss_fwd_f32", ins["real"].ptr(), ins["fake"].ptr(), B_, K, 1.0, *feats, T, J, eps_, 7,
             W.LMIN, W.THRESH, 0, w_, None, Q_, outs["C3"].ptr(), u_, outs["v"].ptr(), outs["cost"].ptr(), outs["nits"].ptr(),
             outs["loss"].ptr(), ws.ptr(), wsb_, None, want=want)

    def lbwd(w_=wq.ptr(), B_=B, Q_=Q, eps_=1.0, u_=outs["u"].ptr(), wsb_=wsb, want=EINVAL):
        call(L, "kccot_conditional_sinkhorn_loss_bwd_f32", g1.ptr(), ins["real"].ptr(), ins["fake"].ptr(), B_, K, 1.0, *feats, T, J,
             eps_, 7, w_, None, Q_, outs["C3"].ptr(), u_, outs["v"].ptr(), outs["nits"].ptr(), outs["dfake"].ptr(),
             outs["dh_fake"].ptr(), outs["dh_real"].ptr(), outs["dm_real"].ptr(), outs["dm_fake"].ptr(), ws.ptr(), wsb_, None,
             want=want)

    for f in (lfwd, lbwd):
        f(w_=None)
        f(B_=0)
        f(Q_=0)
        f(eps_=0.0)
        f(u_=None)
        f(wsb_=need - 4, want=EWORKSPACE)
    assert all(o.untouched() for o in outs.values()) and ws.untouched()


@pytest.mark.parametrize("shape,Q", [LOSS_CASES[0], LOSS_CASES[2]])
def test_loss_entry_points_through_the_abi_give_the_wrappers_bits(L, shape, Q):
    t = loss_inputs(shape, Q)
    B, T, H, Wd, Cc, J = shape
    K = T * H * Wd * Cc
    Lh = LOSS_L
    ins = {k: Buf((B, K) if k in ("real", "fake") else t[k].shape, t[k].reshape(B, -1) if k in ("real", "fake") else t[k])
           for k in ("real", "fake") + FEATS}
    ins["w"], ins["g"] = Buf((Q, B), t["w"]), Buf((1,), torch.ones(1))
    out = {"C3": Buf((3, B, B)), "u": Buf((Q, 3, Lh, B)), "v": Buf((Q, 3, Lh, B)), "cost": Buf((Q, 3)),
           "nits": Buf((2, Q, 3), dtype=I32), "loss": Buf((1,)), "dfake": Buf((B, K)), "dh_fake": Buf((B, T, J)),
           "dh_real": Buf((B, T, J)), "dm_real": Buf((B, T, J)), "dm_fake": Buf((B, T, J))}
    ws, wsb = workspace(L.lib.kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, Q))
    out["ws"] = ws
    feats = [ins[k].ptr() for k in ("h_fake", "h_real", "m_real", "m_fake")]
    call(L, "kccot_conditional_sinkhorn_loss_fwd_f32", ins["real"].ptr(), ins["fake"].ptr(), B, K, W.cases.SC, *feats, T, J, LOSS_EPS,
         LOSS_L, W.LMIN, W.THRESH, 0, ins["w"].ptr(), None, Q, out["C3"].ptr(), out["u"].ptr(), out["v"].ptr(), out["cost"].ptr(),
         out["nits"].ptr(), out["loss"].ptr(), ws.ptr(), wsb, None)
    call(L, "kccot_conditional_sinkhorn_loss_bwd_f32", ins["g"].ptr(), ins["real"].ptr(), ins["fake"].ptr(), B, K, W.cases.SC, *feats,
         T, J, LOSS_EPS, Lh, ins["w"].ptr(), None, Q, out["C3"].ptr(), out["u"].ptr(), out["v"].ptr(), out["nits"].ptr(),
         out["dfake"].ptr(), out["dh_fake"].ptr(), out["dh_real"].ptr(), out["dm_real"].ptr(), out["dm_fake"].ptr(), ws.ptr(), wsb,
         None)
    for k, bf in list(ins.items()) + list(out.items()):
        assert bf.guards_intact(), "guard zone of %s overwritten" % k
    got = run_loss(shape, Q, weights=t["w"])
    for k, g in zip(("loss", "dfake", "dh_fake", "dm_real", "dh_real", "dm_fake"), got):
        assert bool(torch.isfinite(out[k].t).all()), k
        assert same_bits(out[k].t.reshape(-1), g.reshape(-1)), k
    assert out["nits"].t[0].tolist() == [[LOSS_L] * 3] * Q


# ================================================================ 7. trainer
TB, TH, TW, TC, TT, TiT = 2, 64, 64, 1, 6, 2      # the smallest configuration of the trainer tests (tests/test_gpu_bicausal_trainer.py)


def test_trainer_runs_an_iteration_on_the_conditional_loss(monkeypatch):
    from kccotgan_amd import gan, gan_utils
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    tr = KCCOTTrainer(TB, total_time_steps=TT, int_time_steps=TiT, x_height=TH, x_width=TW, channels=TC, kernel="1d", warmup=10,
                      device="cuda:0", conditional_bandwidth=0.2)
    assert tr._loss_tag() == "compute_conditional_sinkhorn_loss"
    seen = []
    orig = gan_utils.kernel_conditional_weights

    def spy(context, bandwidth, queries=None):
        seen.append((tuple(context.shape), float(bandwidth), context.requires_grad, torch.is_grad_enabled()))
        return orig(context, bandwidth, queries)
    monkeypatch.setattr(gan_utils, "kernel_conditional_weights", spy)
    p0 = [torch.cat([p.detach().reshape(-1) for p in ps]).clone() for ps in (tr.g_params, tr.d_params)]
    x = torch.rand(TB, TH, TT, TW, TC, device="cuda:0")
    gan_utils.last_info.clear()
    pm, loss = tr.train_iteration(x)
    assert bool(torch.isfinite(pm)) and bool(torch.isfinite(loss))
    p1 = [torch.cat([p.detach().reshape(-1) for p in ps]) for ps in (tr.g_params, tr.d_params)]
    assert not torch.equal(p0[0], p1[0]) and not torch.equal(p0[1], p1[1])
    info = gan_utils.last_info
    assert tuple(info["compute_conditional_sinkhorn_loss"].shape) == (TB, 3) and "compute_sinkhorn_loss" not in info
    gan_utils.raise_if_solver_aborted((tr._loss_tag(),))
    # once per forward (two forwards per iteration), on the unsmoothed context frames, bandwidth 0.2 sqrt(Kc), no gradient
    kc = TH * TiT * TW * TC
    assert seen == [((TB, TH, TiT, TW, TC), 0.2 * math.sqrt(kc), False, False)] * 2


def test_trainer_refuses_conflicting_options():
    from kccotgan_amd.kernel_train import KCCOTTrainer
    kw = dict(total_time_steps=TT, int_time_steps=TiT, x_height=TH, x_width=TW, channels=TC, device="cuda:0",
              conditional_bandwidth=0.2)
    with pytest.raises(ValueError, match="conditional_bandwidth"):
        KCCOTTrainer(TB, mixed_sinkhorn=True, **kw)
    with pytest.raises(ValueError, match="conditional_bandwidth"):
        KCCOTTrainer(TB, bi_causal=True, **kw)
    with pytest.raises(NotImplementedError, match="sharded_sinkhorn_loss"):
        KCCOTTrainer(TB, group=object(), **kw)
