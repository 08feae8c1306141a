"""The WEIGHT gradients on the device (include/kccot_weight_grad.h, gan_utils.compute_weighted_sinkhorn[_loss] w.r.t. their
weights, gan_utils.compute_kernel_conditional_sinkhorn_loss) held to float64.

Tolerance.  da / db are sums of the reverse sweep's dual adjoints over ALL iterations, divided by weights that span two orders
of magnitude: rounding in the zero-sum mode of the adjoints does not die out, so dC's error is no yardstick for them.  The
yardstick is the plain-torch sweep of tests/test_weight_grad_cpu.py (no code shared with the library) run in float32 against
its own float64 run on the same inputs, per quantity; for the estimator's adjoint and the end-to-end gradients it is the same
formulas evaluated in torch float32 on the CPU.  A device result must satisfy
    |got - ref| <= 4 max(yardstick, 2^-24) max|ref|
with the factor and the floor of tests/test_gpu_weighted_sinkhorn.py (the kernel's v_exp_f32 and its summation order differ
from torch's).  dC, dC3, dfake and the feature gradients of a _dw call must be the BITS of the call without _dw.
Every test prints its figures before it asserts (-s).  Every output and workspace handed to the C ABI lies between NaN-filled
guard zones; workspaces are exactly as long as the queries say.
"""
import functools
import math

import numpy as np
import pytest
import torch

import test_conditional_sinkhorn_cpu as CC
import test_gpu_conditional_sinkhorn as GC
import test_gpu_weighted_sinkhorn as GW
import test_weight_grad_cpu as WG
import test_weighted_sinkhorn_cpu as W
from test_gpu_weighted_sinkhorn import Buf, call, rel_err, same_bits, within, workspace, GCOST, FEATS
from test_weighted_sinkhorn_cpu import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
I32 = torch.int32
COEF = CC.COEF


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


# ================================================================ 6. solver da / db through the ABI against float64
@functools.lru_cache(maxsize=None)
def solver_reference(n, eps, Lit):
    """float64 autograd of sum_p GCOST[p] W(C_p; a_p, b_p) w.r.t. a, b [3,n], on the float32 inputs the device reads."""
    C, a, b = GW.problems(n)
    al, bl = a.double().requires_grad_(True), b.double().requires_grad_(True)
    tot = sum(GCOST[p] * W.weighted_sinkhorn(C[p].double(), al[p], bl[p], eps, Lit)[0] for p in range(3))
    return torch.autograd.grad(tot, (al, bl))


@functools.lru_cache(maxsize=None)
def solver_yardstick(n, eps, Lit):
    """The torch sweep in float32 against itself in float64: relative errors of (da, db) over the three problems."""
    C, a, b = GW.problems(n)
    r = [WG.sweep(C[p], a[p], b[p], eps, Lit, g=GCOST[p]) for p in range(3)]
    s = [WG.sweep(C[p], a[p], b[p], eps, Lit, g=GCOST[p], dtype=F32) for p in range(3)]
    return tuple(rel_err(torch.stack([x[k] for x in s]), torch.stack([x[k] for x in r])) for k in (3, 4))


def solve_dw(L, C, a, b, eps, Lit, gcost=GCOST, c_off=0, Lmin=W.LMIN, stop_mode=0):
    """dC of kccot_sinkhorn_weighted_bwd_f32, then (dC, da, db) of kccot_sinkhorn_weighted_bwd_dw_f32 on the same forward; the
    forward's cost, both rows of nits and the whole (NaN-prefilled) histories come back too.  c_off: as GW.solve."""
    nprob, n, _ = C.shape
    Lh = max(Lit, 1)
    bufs = {"C": GW.OffsetBuf(C.shape, C, c_off), "a": Buf(a.shape, a), "b": Buf(b.shape, b), "u": Buf((nprob, Lh, n)),
            "v": Buf((nprob, Lh, n)),
            "cost": Buf((nprob,)), "nits": Buf((2 * nprob,), dtype=I32), "dC0": Buf(C.shape), "dC": Buf(C.shape),
            "da": Buf((nprob, n)), "db": Buf((nprob, n)), "g": Buf((nprob,), torch.tensor(gcost[:nprob]))}
    ws, wsb = workspace(L.lib.kccot_sinkhorn_workspace_bytes(nprob, n))
    bufs["ws"] = ws
    wp = ws.ptr() if wsb else None
    call(L, "kccot_sinkhorn_weighted_fwd_f32", bufs["C"].ptr(), bufs["a"].ptr(), bufs["b"].ptr(), nprob, n, eps, Lit, Lmin,
         W.THRESH, stop_mode, bufs["u"].ptr(), bufs["v"].ptr(), bufs["cost"].ptr(), bufs["nits"].ptr(), None, wp, wsb, None)
    call(L, "kccot_sinkhorn_weighted_bwd_f32", bufs["C"].ptr(), bufs["a"].ptr(), bufs["b"].ptr(), bufs["u"].ptr(),
         bufs["v"].ptr(), bufs["nits"].ptr(), nprob, n, eps, Lh, bufs["g"].ptr(), bufs["dC0"].ptr(), wp, wsb, None)
    call(L, "kccot_sinkhorn_weighted_bwd_dw_f32", bufs["C"].ptr(), bufs["a"].ptr(), bufs["b"].ptr(), bufs["u"].ptr(),
         bufs["v"].ptr(), bufs["nits"].ptr(), nprob, n, eps, Lh, bufs["g"].ptr(), bufs["dC"].ptr(), bufs["da"].ptr(),
         bufs["db"].ptr(), wp, wsb, None)
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d)" % (k, n)
    return {k: bufs[k].t.clone() for k in ("nits", "dC0", "dC", "da", "db", "cost", "u", "v")}


@pytest.mark.parametrize("eps,Lit", [(0.8, 7), (1.0, 100)])
@pytest.mark.parametrize("n", GW.SIZES)
def test_solver_weight_gradients_against_fp64(L, n, eps, Lit):
    C, a, b = GW.problems(n)
    ref_a, ref_b = solver_reference(n, eps, Lit)
    ya, yb = solver_yardstick(n, eps, Lit)
    out = solve_dw(L, C, a, b, eps, Lit)
    assert out["nits"][:3].tolist() == [Lit] * 3
    assert same_bits(out["dC"], out["dC0"]), "dC of the _dw call differs from kccot_sinkhorn_weighted_bwd_f32"
    r1 = within("n=%d eps=%g L=%d da" % (n, eps, Lit), out["da"], ref_a, ya)
    r2 = within("n=%d eps=%g L=%d db" % (n, eps, Lit), out["db"], ref_b, yb)
    print("WORST n=%d: %.2f" % (n, max(r1, r2)))


def test_one_iteration_and_weight_gradient_bits_do_not_depend_on_nprob(L):
    """L = 1 (the adjoint of v_0 is not added) on both solvers, and one problem alone gives the bits it gives among three."""
    for n in (64, 130):
        C, a, b = GW.problems(n)
        ref_a, ref_b = solver_reference(n, 1.0, 1)
        ya, yb = solver_yardstick(n, 1.0, 1)
        full = solve_dw(L, C, a, b, 1.0, 1)
        within("n=%d L=1 da" % n, full["da"], ref_a, ya)
        within("n=%d L=1 db" % n, full["db"], ref_b, yb)
        one = solve_dw(L, C[1:2].contiguous(), a[1:2].contiguous(), b[1:2].contiguous(), 1.0, 1, gcost=GCOST[1:2])
        assert same_bits(one["da"][0], full["da"][1]) and same_bits(one["db"][0], full["db"][1])


# ================================================================ 7. the weighted loss through autograd
def _loss_weight_grads(shape, dtype, normalize, scale, Lit=GW.LOSS_L):
    """(dw_real, dw_fake) of the weighted loss by the torch sweep in `dtype`: cost matrices, three sweeps with g = {2,-1,-1},
    dw_real = da_xy + (da_xx + db_xx), dw_fake = db_xy + (da_yy + db_yy), then the normalisation's own adjoint."""
    t = GW.loss_inputs(shape)
    B = shape[0]
    d = {k: t[k].to(dtype) for k in ("real", "fake") + FEATS}
    x, y = d["real"].reshape(B, 1, -1), d["fake"].reshape(B, 1, -1)
    C3 = [W.ot.modified_cost(x, y, d["h_fake"], d["m_real"], W.cases.SC), W.ot.modified_cost(x, x, d["h_real"], d["m_real"], W.cases.SC),
          W.ot.modified_cost(y, y, d["h_fake"], d["m_fake"], W.cases.SC)]
    wr, wf = (t["w_real"] * scale).to(dtype), (t["w_fake"] * scale).to(dtype)
    a, b = (wr / wr.sum(), wf / wf.sum()) if normalize else (wr, wf)
    xy = WG.sweep(C3[0], a, b, GW.LOSS_EPS, Lit, g=2.0, dtype=dtype)
    xx = WG.sweep(C3[1], a, a, GW.LOSS_EPS, Lit, g=-1.0, dtype=dtype)
    yy = WG.sweep(C3[2], b, b, GW.LOSS_EPS, Lit, g=-1.0, dtype=dtype)
    da, db = xy[3] + (xx[3] + xx[4]), xy[4] + (yy[3] + yy[4])
    if normalize:        # a = w / s: dw = (da - <da, a>) / s
        da, db = (da - (da * a).sum()) / wr.sum(), (db - (db * b).sum()) / wf.sum()
    return da, db


@functools.lru_cache(maxsize=None)
def loss_weight_reference(shape, normalize, scale, Lit=GW.LOSS_L):
    """float64 autograd of W.weighted_loss (with the normalisation) w.r.t. w_real, w_fake, and the yardsticks."""
    t = GW.loss_inputs(shape)
    d = {k: t[k].double() for k in ("real", "fake") + FEATS}
    wr, wf = (t["w_real"] * scale).double().requires_grad_(True), (t["w_fake"] * scale).double().requires_grad_(True)
    a, b = (wr / wr.sum(), wf / wf.sum()) if normalize else (wr, wf)
    loss, _, nits = W.weighted_loss(d["real"], d["fake"], W.cases.SC, GW.LOSS_EPS, Lit, d["h_fake"], d["m_real"], d["h_real"],
                                    d["m_fake"], a, b)
    assert nits == (Lit,) * 3
    ref = torch.autograd.grad(loss, (wr, wf))
    r64, r32 = _loss_weight_grads(shape, F64, normalize, scale, Lit), _loss_weight_grads(shape, F32, normalize, scale, Lit)
    for x, y in zip(r64, ref):                       # the sweep composition IS the gradient (float64 against float64)
        assert rel_err(x, y) <= 1e-9
    return ref, tuple(rel_err(x, y) for x, y in zip(r32, r64))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", GW.LOSS_SHAPES)
def test_weighted_loss_weight_gradients_through_autograd(shape, normalize):
    from kccotgan_amd import gan_utils as g
    t = GW.loss_inputs(shape)
    scale = 7.3 if normalize else 1.0
    ref, yard = loss_weight_reference(shape, normalize, scale)
    real = t["real"].to(DEV)
    outs = []
    for with_w in (False, True):
        leaves = [t[k].to(DEV).requires_grad_(True) for k in ("fake",) + FEATS]
        fake, hf, mr, hr, mf = leaves
        wr, wf = (t["w_real"] * scale).to(DEV).requires_grad_(with_w), (t["w_fake"] * scale).to(DEV).requires_grad_(with_w)
        loss = g.compute_weighted_sinkhorn_loss(real, fake, W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, hf, mr, hr, mf, wr, wf,
                                                normalize=normalize)
        outs.append((loss.detach(),) + torch.autograd.grad(loss, leaves + ([wr, wf] if with_w else [])))
    torch.cuda.synchronize()
    plain, dw = outs
    for k, x, y in zip(GW.NAMES, plain, dw):
        assert same_bits(x.reshape(-1), y.reshape(-1)), "%s changes when the weights require a gradient" % k
    r1 = within("%s normalize=%s dw_real" % (shape, normalize), dw[6], ref[0], yard[0])
    r2 = within("%s normalize=%s dw_fake" % (shape, normalize), dw[7], ref[1], yard[1])
    print("WORST loss dw %s normalize=%s: %.2f" % (shape, normalize, max(r1, r2)))


def test_compute_weighted_sinkhorn_differentiates_its_marginals():
    from kccotgan_amd import gan_utils as g
    n = 67
    rng = np.random.default_rng(3)
    x, y = (torch.from_numpy(rng.random((n, 3, 4), dtype=np.float32)).to(DEV) for _ in range(2))
    h, M = (torch.from_numpy(rng.random((n, 3, 2), dtype=np.float32)).to(DEV) for _ in range(2))
    mu, nu = W.random_weights(n, 5).float(), W.random_weights(n, 6).float()
    mud, nud = mu.to(DEV).requires_grad_(True), nu.to(DEV).requires_grad_(True)
    cost = g.compute_weighted_sinkhorn(x, y, h, M, 1.0, mud, nud, epsilon=1.0, L=20)
    da, db = torch.autograd.grad(cost, (mud, nud))
    C = W.ot.modified_cost(x.double().cpu(), y.double().cpu(), h.double().cpu(), M.double().cpu(), 1.0)
    r = WG.sweep(C, mu, nu, 1.0, 20)
    s = WG.sweep(C.float(), mu, nu, 1.0, 20, dtype=F32)
    within("compute_weighted_sinkhorn dmu", da, r[3], rel_err(s[3], r[3]))
    within("compute_weighted_sinkhorn dnu", db, r[4], rel_err(s[4], r[4]))


# ================================================================ 8. the conditional solver
COND_EPS_L = (1.0, 100)
GLOSS = (1.0, -0.5)


@functools.lru_cache(maxsize=None)
def cond_pieces(n, dtype):
    """Per (q, k) of GC.problem(n): cost and da + db of W(C3[k]; w_q, w_q) at g = 1 by the torch sweep in `dtype`."""
    C3, w, _ = GC.problem(n)
    eps, Lit = COND_EPS_L
    cost = torch.zeros(GC.QMAX, 3, dtype=dtype)
    dw = torch.zeros(GC.QMAX, 3, n, dtype=dtype)
    for q in range(GC.QMAX):
        for k in range(3):
            r = WG.sweep(C3[k], w[q], w[q], eps, Lit, dtype=dtype)
            cost[q, k], dw[q, k] = r[0], r[3] + r[4]
    return cost, dw


def cond_combine(pieces, omega, Q, gloss):
    """(dw [Q,n], domega [Q]) from per-problem pieces, in the pieces' dtype."""
    cost, dw = pieces
    dt = cost.dtype
    om = (torch.full((Q,), 1.0 / Q, dtype=F64) if omega is None else omega.double()).to(dt)
    coef = torch.tensor(COEF, dtype=dt)
    return (gloss * om[:, None] * (coef[None, :, None] * dw[:Q]).sum(1), gloss * (coef[None, :] * cost[:Q]).sum(1))


@functools.lru_cache(maxsize=None)
def cond_autograd(n, Q, given):
    """float64 autograd of the conditional loss (gloss = 1) w.r.t. the weight rows and the query weights."""
    C3, w, omega = GC.problem(n)
    eps, Lit = COND_EPS_L
    wl = w[:Q].double().requires_grad_(True)
    om = ((omega[:Q] / omega[:Q].sum()).contiguous().double() if given else torch.full((Q,), 1.0 / Q, dtype=F64)).requires_grad_(True)
    loss, _, _ = CC.conditional_loss_from_costs(C3.double(), wl, om, eps, Lit)
    return torch.autograd.grad(loss, (wl, om))


def cond_solve_dw(L, C3, w, omega, eps, Lit, gloss, want_domega=True, Lmin=W.LMIN):
    Q, n = w.shape
    Lh = max(Lit, 1)
    bufs = {"C3": Buf(C3.shape, C3), "w": Buf(w.shape, w), "u": Buf((Q, 3, Lh, n)), "v": Buf((Q, 3, Lh, n)), "cost": Buf((Q, 3)),
            "nits": Buf((2, Q, 3), dtype=I32), "loss": Buf((1,)), "dC0": Buf(C3.shape), "dC3": Buf(C3.shape), "dw": Buf((Q, n)),
            "dom": Buf((Q,)), "g": Buf((1,), torch.tensor([gloss]))}
    if omega is not None:
        bufs["omega"] = Buf((Q,), omega)
    op = bufs["omega"].ptr() if omega is not None else None
    ws0, wsb0 = workspace(L.lib.kccot_sinkhorn_conditional_workspace_bytes(Q, n))
    ws, wsb = workspace(L.lib.kccot_sinkhorn_conditional_dw_workspace_bytes(Q, n))
    assert wsb > wsb0 > 0
    bufs["ws0"], bufs["ws"] = ws0, ws
    call(L, "kccot_sinkhorn_conditional_fwd_f32", bufs["C3"].ptr(), bufs["w"].ptr(), op, Q, n, eps, Lit, Lmin, W.THRESH,
         bufs["u"].ptr(), bufs["v"].ptr(), bufs["cost"].ptr(), bufs["nits"].ptr(), bufs["loss"].ptr(), ws0.ptr(), wsb0, None)
    call(L, "kccot_sinkhorn_conditional_bwd_f32", bufs["g"].ptr(), bufs["C3"].ptr(), bufs["w"].ptr(), op, bufs["u"].ptr(),
         bufs["v"].ptr(), bufs["nits"].ptr(), Q, n, eps, Lh, bufs["dC0"].ptr(), ws0.ptr(), wsb0, None)
    call(L, "kccot_sinkhorn_conditional_bwd_dw_f32", bufs["g"].ptr(), bufs["C3"].ptr(), bufs["w"].ptr(), op, bufs["u"].ptr(),
         bufs["v"].ptr(), bufs["nits"].ptr(), Q, n, eps, Lh, bufs["dC3"].ptr(), bufs["cost"].ptr(), bufs["dw"].ptr(),
         bufs["dom"].ptr() if want_domega else None, ws.ptr(), wsb, None)
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d Q=%d)" % (k, n, Q)
    if not want_domega:
        assert bufs["dom"].untouched()
    return {k: bufs[k].t.clone() for k in ("nits", "cost", "dC0", "dC3", "dw", "dom", "loss", "u", "v")}


@pytest.mark.parametrize("Q", [1, 7])
@pytest.mark.parametrize("n", (5, 67, 130))
def test_conditional_solver_weight_gradients_against_fp64(L, n, Q):
    C3, w, omega = GC.problem(n)
    w = w[:Q].contiguous()
    eps, Lit = COND_EPS_L
    p64, p32 = cond_pieces(n, F64), cond_pieces(n, F32)
    worst = 0.0
    for given in (False, True):
        om = (omega[:Q] / omega[:Q].sum()).contiguous() if given else None
        auto_dw, auto_dom = cond_autograd(n, Q, given)
        for gl in GLOSS:
            tag = "n=%d Q=%d omega=%s gloss=%g" % (n, Q, "given" if given else "1/Q", gl)
            ref_dw, ref_dom = cond_combine(p64, om, Q, gl)
            assert rel_err(ref_dw, gl * auto_dw) <= 1e-9 and rel_err(ref_dom, gl * auto_dom) <= 1e-9    # float64 against float64
            y_dw, y_dom = cond_combine(p32, om, Q, gl)
            out = cond_solve_dw(L, C3, w, om, eps, Lit, gl)
            assert out["nits"][0].tolist() == [[Lit] * 3] * Q
            assert same_bits(out["dC3"], out["dC0"]), tag + ": dC3 differs from kccot_sinkhorn_conditional_bwd_f32"
            worst = max(worst, within(tag + " dw", out["dw"], gl * auto_dw, rel_err(y_dw, ref_dw)))
            worst = max(worst, within(tag + " domega", out["dom"], gl * auto_dom, rel_err(y_dom, ref_dom)))
    none = cond_solve_dw(L, C3, w, None, eps, Lit, 1.0, want_domega=False)             # domega_out = NULL is accepted
    assert bool(torch.isfinite(none["dw"]).all())
    print("WORST conditional dw n=%d: %.2f" % (n, worst))


# ================================================================ 9. the adjoint of the weight estimator
def weights_bwd_abi(L, D, w, dw, bw, dev=False):
    Q, n = D.shape
    b = {"D": Buf(D.shape, D), "w": Buf(w.shape, w), "dw": Buf(dw.shape, dw), "dD": Buf((Q, n)), "dbw": Buf((Q,)),
         "bw": Buf((1,), torch.tensor([bw]))}
    if dev:
        call(L, "kccot_conditional_weights_bwd_dev_f32", b["D"].ptr(), b["w"].ptr(), b["dw"].ptr(), Q, n, b["bw"].ptr(),
             b["dD"].ptr(), b["dbw"].ptr(), None)
    else:
        call(L, "kccot_conditional_weights_bwd_f32", b["D"].ptr(), b["w"].ptr(), b["dw"].ptr(), Q, n, bw, b["dD"].ptr(),
             b["dbw"].ptr(), None)
    assert all(x.guards_intact() for x in b.values())
    return b["dD"].t.clone(), b["dbw"].t.clone()


def weights_fwd_abi(L, D, bw, dev=False):
    Q, n = D.shape
    Db, out, bwb = Buf(D.shape, D), Buf((Q, n)), Buf((1,), torch.tensor([bw]))
    if dev:
        call(L, "kccot_conditional_weights_dev_f32", Db.ptr(), Q, n, bwb.ptr(), out.ptr(), None)
    else:
        call(L, "kccot_conditional_weights_f32", Db.ptr(), Q, n, bw, out.ptr(), None)
    assert Db.guards_intact() and out.guards_intact()
    return out.t.clone()


@pytest.mark.parametrize("Q,n", [(3, 5), (7, 130), (5, 1024)])
def test_weights_adjoint_kernel_against_fp64(L, Q, n):
    D = GC.distances(Q, n)
    dw = torch.randn(Q, n, generator=torch.Generator().manual_seed(Q + n))
    pos = D[D > 0].sort().values
    # every entry live (max logit 50, as the sibling test); most entries floored (logit 66 at the 20 % quantile of D: softmax
    # mass < 2^-100 = e^-69.3 from ~1.05 x that distance on) while each row keeps its own sample and the nearest others
    cases = (("live", float(np.float32(math.sqrt(float(D.max()) / 100.0) * (1.0 + 1e-6)))),
             ("floored", float(np.float32(math.sqrt(float(pos[int(0.2 * len(pos))]) / 132.0)))))
    for name, bw in cases:
        w = weights_fwd_abi(L, D, bw)
        assert same_bits(w, weights_fwd_abi(L, D, bw, dev=True)), "bandwidth from device memory: other weight bits"
        wc = w.cpu()
        floored = wc == 2.0 ** -100
        if name == "live":
            assert not bool(floored.any())
        else:
            assert float(floored.float().mean()) > 0.5 and bool((~floored).sum(1).min() >= 1)
        ref_dD, ref_dbw = WG.weights_adjoint(D, wc, dw, bw)
        y_dD, y_dbw = WG.weights_adjoint(D, wc, dw, bw, dtype=F32)
        dD, dbw = weights_bwd_abi(L, D, wc, dw, bw)
        dD2, dbw2 = weights_bwd_abi(L, D, wc, dw, bw, dev=True)
        assert same_bits(dD, dD2) and same_bits(dbw, dbw2), "bandwidth from device memory: other gradient bits"
        tag = "weights adjoint Q=%d n=%d %s" % (Q, n, name)
        within(tag + " dD", dD, ref_dD, rel_err(y_dD, ref_dD))
        within(tag + " dbw", dbw.double().sum().reshape(()), ref_dbw.sum().reshape(()),
               rel_err(y_dbw.sum().reshape(()), ref_dbw.sum().reshape(())))
        assert bool((dD.cpu()[floored] == 0).all()), "a floored entry has a gradient"


# ================================================================ 10. end to end
E2E = [((6, 4, 8, 8, 1, 3), None), ((64, 5, 8, 8, 1, 4), (3, 60, 17, 0, 41))]      # shape, queries
E2E_BW = 1.7


@functools.lru_cache(maxsize=None)
def e2e_inputs(shape):
    t = dict(GW.loss_inputs(shape))
    B = shape[0]
    rng = np.random.default_rng(99 + B)
    t["context"] = torch.from_numpy(rng.random((B, 2, 3, 4), dtype=np.float32))
    return t


def e2e_torch(shape, queries, dtype):
    """(loss, dbandwidth, dcontext, dquery_weights) in torch `dtype` on the CPU: squared distances, CC.conditional_weights'
    formula, CC.conditional_loss, autograd."""
    t = e2e_inputs(shape)
    B = shape[0]
    d = {k: t[k].to(dtype) for k in ("real", "fake") + FEATS}
    c = t["context"].to(dtype).clone().requires_grad_(True)      # a copy: .to(float32) would hand back the cached input itself
    bw = torch.tensor(E2E_BW, dtype=dtype, requires_grad=True)
    Q = B if queries is None else len(queries)
    om = W.random_weights(Q, 5 + Q).to(dtype).requires_grad_(True)
    cf = c.reshape(B, -1)
    cq = cf if queries is None else cf[list(queries)]
    D = ((cq[:, None, :] - cf[None, :, :]) ** 2).sum(-1)
    w = torch.clamp_min(torch.softmax(-D / (2.0 * bw * bw), dim=1), CC.FLOOR_W)
    loss = CC.conditional_loss(d["real"], d["fake"], W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, d["h_fake"], d["m_real"], d["h_real"],
                               d["m_fake"], w, om)
    return (loss.detach(),) + torch.autograd.grad(loss, (bw, c, om))


@functools.lru_cache(maxsize=None)
def e2e_reference(shape, queries):
    r64, r32 = e2e_torch(shape, queries, F64), e2e_torch(shape, queries, F32)
    return r64, tuple(rel_err(x.reshape(-1), y.reshape(-1)) for x, y in zip(r32, r64))


def e2e_device(shape, queries, new_leaves=True):
    """loss and gradients of compute_kernel_conditional_sinkhorn_loss; returns the step function's tensors."""
    from kccotgan_amd import gan_utils as g
    t = e2e_inputs(shape)
    Q = shape[0] if queries is None else len(queries)
    assert not t["context"].requires_grad
    real = t["real"].to(DEV)
    fake = t["fake"].to(DEV).requires_grad_(True)
    feats = [t[k].to(DEV) for k in FEATS]
    ctx = t["context"].detach().to(DEV).requires_grad_(new_leaves)      # a leaf on the device, like every other input
    bw = torch.tensor(E2E_BW, device=DEV).requires_grad_(new_leaves)
    om = W.random_weights(Q, 5 + Q).float().to(DEV).requires_grad_(new_leaves)
    qi = None if queries is None else torch.tensor(queries, device=DEV)

    def step():
        loss = g.compute_kernel_conditional_sinkhorn_loss(real, fake, W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, *feats, ctx, bw, qi, om)
        return (loss,) + torch.autograd.grad(loss, [fake] + ([bw, ctx, om] if new_leaves else []))

    return step, (real, fake, feats, ctx, bw, om, qi)


@pytest.mark.parametrize("shape,queries", E2E)
def test_end_to_end_against_fp64(shape, queries):
    from kccotgan_amd import gan_utils as g
    ref, yard = e2e_reference(shape, queries)
    step, (real, fake, feats, ctx, bw, om, qi) = e2e_device(shape, queries)
    loss, dfake, dbw, dctx, dom = step()
    torch.cuda.synchronize()
    tag = "compute_kernel_conditional_sinkhorn_loss"
    B, Q = shape[0], om.shape[0]
    info = g.last_info
    assert tuple(info[tag].shape) == (Q, 3) and info[tag].tolist() == [[GW.LOSS_L] * 3] * Q
    assert tuple(info[tag + "_executed"].shape) == (Q, 3) and tuple(info[tag + "_costs"].shape) == (Q, 3)
    assert tuple(info[tag + "_C3"].shape) == (3, B, B) and info[tag + "_fused_sweep"] is False and info[tag + "_path"] == "register"
    g.raise_if_solver_aborted((tag,))
    worst = 0.0
    for name, got, r, y in zip(("loss", "dbandwidth", "dcontext", "dquery_weights"), (loss.detach(), dbw, dctx, dom), ref, yard):
        worst = max(worst, within("%s Q=%d %s" % (shape, Q, name), got.reshape(-1), r.reshape(-1), y))
    print("WORST end to end %s: %.2f" % (shape, worst))
    # nothing new requires a gradient: the bits of the existing two-call composition (float bandwidth and tensor bandwidth)
    step0, (real, fake0, feats, ctx0, bw0, om0, qi) = e2e_device(shape, queries, new_leaves=False)
    loss0, dfake0 = step0()
    fake1 = fake0.detach().clone().requires_grad_(True)
    wts = g.kernel_conditional_weights(ctx0, E2E_BW, qi)
    loss1 = g.compute_conditional_sinkhorn_loss(real, fake1, W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, *feats, wts, om0)
    (dfake1,) = torch.autograd.grad(loss1, fake1)
    fake2 = fake0.detach().clone().requires_grad_(True)
    loss2 = g.compute_kernel_conditional_sinkhorn_loss(real, fake2, W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, *feats, ctx0, E2E_BW, qi, om0)
    (dfake2,) = torch.autograd.grad(loss2, fake2)
    torch.cuda.synchronize()
    for lo, df in ((loss0, dfake0), (loss2, dfake2), (loss.detach(), dfake)):
        assert same_bits(lo.detach().reshape(-1), loss1.detach().reshape(-1)) and same_bits(df, dfake1)


# ================================================================ 11. poisoning is per query
def test_a_bad_weight_gives_nan_dw_for_its_query_only(L):
    n, Q = 64, 3
    C3, w, _ = GC.problem(n)
    w = w[:Q].contiguous()
    good = cond_solve_dw(L, C3, w, None, 1.0, 7, 1.0)
    w2 = w.clone()
    w2[1, n // 3], w2[1, n // 2] = 0.0, float("nan")
    out = cond_solve_dw(L, C3, w2, None, 1.0, 7, 1.0)
    assert out["nits"][0, 1].tolist() == [-1] * 3
    assert bool(torch.isnan(out["dw"][1]).all()) and bool(torch.isnan(out["dom"][1]))
    for q in (0, 2):
        assert same_bits(out["dw"][q], good["dw"][q]) and same_bits(out["dom"][q], good["dom"][q])
        assert bool(torch.isfinite(out["dw"][q]).all())
    # the streaming solver's sweep too
    n = 130
    C3, w, _ = GC.problem(n)
    w2 = w[:2].clone()
    w2[0, 7] = 0.0
    good = cond_solve_dw(L, C3, w[:2].contiguous(), None, 1.0, 7, 1.0)
    out = cond_solve_dw(L, C3, w2, None, 1.0, 7, 1.0)
    assert bool(torch.isnan(out["dw"][0]).all()) and same_bits(out["dw"][1], good["dw"][1])


def test_raise_if_solver_aborted_works_with_the_new_tag(L):
    from kccotgan_amd import gan_utils as g
    shape, queries = E2E[0]
    t = e2e_inputs(shape)
    real, fake = t["real"].to(DEV), t["fake"].to(DEV).requires_grad_(True)
    feats = [t[k].to(DEV) for k in FEATS]
    ctx = t["context"].to(DEV).requires_grad_(True)
    bad = torch.tensor(-1.0, device=DEV, requires_grad=True)        # cannot be refused without reading it: NaN weights
    loss = g.compute_kernel_conditional_sinkhorn_loss(real, fake, W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, *feats, ctx, bad)
    dfake, dctx = torch.autograd.grad(loss, (fake, ctx))
    assert not bool(torch.isfinite(loss)) and not bool(torch.isfinite(dctx).any())
    with pytest.raises(L.KccotError, match="weight"):
        g.raise_if_solver_aborted(("compute_kernel_conditional_sinkhorn_loss",))
    g.compute_kernel_conditional_sinkhorn_loss(real, fake, W.cases.SC, GW.LOSS_EPS, GW.LOSS_L, *feats, ctx, E2E_BW)
    g.raise_if_solver_aborted(("compute_kernel_conditional_sinkhorn_loss",))


# ================================================================ 12. graph replay
def test_forward_and_backward_replay_from_a_graph_bit_for_bit():
    """Nothing is allocated by the library, nothing synchronises, the bandwidth is read on the device: the step of test 10
    (gradients w.r.t. fake, bandwidth, context, query weights) captured once replays to the eager bits, twice."""
    shape, queries = E2E[0]
    step, _ = e2e_device(shape, queries)
    eager = [x.detach().clone() for x in step()]
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
        for k, a, b in zip(("loss", "dfake", "dbandwidth", "dcontext", "dquery_weights"), out, eager):
            assert same_bits(a.detach().reshape(-1), b.reshape(-1)), k


# ================================================================ 13. rejected calls leave everything untouched
def test_rejected_calls_leave_every_output_untouched(L):
    EINVAL, EWORKSPACE, EUNSUPPORTED = L.EINVAL, L.EWORKSPACE, L.EUNSUPPORTED
    for n in (64, 130):
        C, a, b = GW.problems(n)
        nprob, Lit = 3, 7
        Cb, ab, bb, gb = Buf(C.shape, C), Buf(a.shape, a), Buf(b.shape, b), Buf((nprob,), torch.tensor(GCOST))
        hist = {k: Buf((nprob, Lit, n), torch.zeros(nprob, Lit, n)) for k in ("u", "v")}
        nits = Buf((2 * nprob,), torch.full((2 * nprob,), Lit, dtype=I32), I32)
        outs = {k: Buf(s) for k, s in (("dC", C.shape), ("da", (nprob, n)), ("db", (nprob, n)))}
        need = L.lib.kccot_sinkhorn_workspace_bytes(nprob, n)
        ws, wsb = workspace(need)
        wp = ws.ptr() if need else None

        def sb(a_=ab.ptr(), b_=bb.ptr(), n_=n, eps_=1.0, L_=Lit, da_=outs["da"].ptr(), db_=outs["db"].ptr(), wsb_=wsb, want=EINVAL):
            call(L, "kccot_sinkhorn_weighted_bwd_dw_f32", Cb.ptr(), a_, b_, hist["u"].ptr(), hist["v"].ptr(), nits.ptr(), nprob, n_,
                 eps_, L_, gb.ptr(), outs["dC"].ptr(), da_, db_, wp, wsb_, None, want=want)

        for kw in ({"a_": None}, {"b_": None}, {"da_": None}, {"db_": None}, {"n_": 0}, {"eps_": 0.0}, {"L_": -1}):
            sb(**kw)
        sb(n_=1025, wsb_=1 << 40, want=EUNSUPPORTED)
        if need:
            sb(wsb_=need - 4, want=EWORKSPACE)
        assert all(o.untouched() for o in outs.values()) and ws.untouched()

        C3, w, omega = GC.problem(n)
        Q = 3
        w = w[:Q].contiguous()
        C3b, wb, g1 = Buf(C3.shape, C3), Buf(w.shape, w), Buf((1,), torch.ones(1))
        hq = {k: Buf((Q, 3, Lit, n), torch.zeros(Q, 3, Lit, n)) for k in ("u", "v")}
        nq = Buf((2, Q, 3), torch.full((2, Q, 3), Lit, dtype=I32), I32)
        cost = Buf((Q, 3), torch.ones(Q, 3))
        outs = {k: Buf(s) for k, s in (("dC3", C3.shape), ("dw", (Q, n)), ("dom", (Q,)))}
        need = L.lib.kccot_sinkhorn_conditional_dw_workspace_bytes(Q, n)
        ws, wsb = workspace(need)

        def cb(g_=g1.ptr(), w_=wb.ptr(), Q_=Q, n_=n, eps_=1.0, L_=Lit, cost_=cost.ptr(), dw_=outs["dw"].ptr(), wsb_=wsb, want=EINVAL):
            call(L, "kccot_sinkhorn_conditional_bwd_dw_f32", g_, C3b.ptr(), w_, None, hq["u"].ptr(), hq["v"].ptr(), nq.ptr(), Q_, n_,
                 eps_, L_, outs["dC3"].ptr(), cost_, dw_, outs["dom"].ptr(), ws.ptr(), wsb_, None, want=want)

        for kw in ({"g_": None}, {"w_": None}, {"cost_": None}, {"dw_": None}, {"Q_": 0}, {"n_": 0}, {"eps_": 0.0}, {"eps_": -1.0},
                   {"L_": -1}):
            cb(**kw)
        cb(n_=1025, want=EUNSUPPORTED)
        cb(wsb_=need - 4, want=EWORKSPACE)
        cb(wsb_=L.lib.kccot_sinkhorn_conditional_workspace_bytes(Q, n), want=EWORKSPACE)      # enough without dw only
        assert all(o.untouched() for o in outs.values()) and ws.untouched()
    # the estimator's adjoint and the device-bandwidth forward
    D = GC.distances(3, 5)
    Db, wv, dwv, bwb = Buf(D.shape, D), Buf(D.shape, torch.full(D.shape, 0.2)), Buf(D.shape, torch.ones(D.shape)), Buf((1,), torch.ones(1))
    dD, dbw, wout = Buf(D.shape), Buf((3,)), Buf(D.shape)
    for args, want in (((None, wv.ptr(), dwv.ptr(), 3, 5, 1.0, dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), None, dwv.ptr(), 3, 5, 1.0, dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), None, 3, 5, 1.0, dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 3, 5, 1.0, None, dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 3, 5, 1.0, dD.ptr(), None), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 0, 5, 1.0, dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 3, 0, 1.0, dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 3, 5, 0.0, dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 3, 5, float("nan"), dD.ptr(), dbw.ptr()), EINVAL),
                       ((Db.ptr(), wv.ptr(), dwv.ptr(), 3, 1025, 1.0, dD.ptr(), dbw.ptr()), EUNSUPPORTED)):
        call(L, "kccot_conditional_weights_bwd_f32", *args, None, want=want)
    call(L, "kccot_conditional_weights_bwd_dev_f32", Db.ptr(), wv.ptr(), dwv.ptr(), 3, 5, None, dD.ptr(), dbw.ptr(), None, want=EINVAL)
    call(L, "kccot_conditional_weights_bwd_dev_f32", Db.ptr(), wv.ptr(), dwv.ptr(), 3, 1025, bwb.ptr(), dD.ptr(), dbw.ptr(), None,
         want=EUNSUPPORTED)
    call(L, "kccot_conditional_weights_dev_f32", Db.ptr(), 3, 5, None, wout.ptr(), None, want=EINVAL)
    call(L, "kccot_conditional_weights_dev_f32", Db.ptr(), 0, 5, bwb.ptr(), wout.ptr(), None, want=EINVAL)
    call(L, "kccot_conditional_weights_dev_f32", Db.ptr(), 3, 1025, bwb.ptr(), wout.ptr(), None, want=EUNSUPPORTED)
    assert dD.untouched() and dbw.untouched() and wout.untouched()
    # the two loss-level backwards
    shape = GW.LOSS_SHAPES[0]
    t = GW.loss_inputs(shape)
    B, T, H, Wd, Cc, J = shape
    K, Q = T * H * Wd * Cc, 4
    ins = {k: Buf((B, K) if k in ("real", "fake") else t[k].shape, t[k].reshape(B, -1) if k in ("real", "fake") else t[k])
           for k in ("real", "fake") + FEATS}
    feats = [ins[k].ptr() for k in ("h_fake", "h_real", "m_real", "m_fake")]
    wr, wf, g1 = Buf((B,), t["w_real"]), Buf((B,), t["w_fake"]), Buf((1,), torch.ones(1))
    C3 = Buf((3, B, B), torch.ones(3, B, B))
    h3 = {k: Buf((3, 7, B), torch.zeros(3, 7, B)) for k in ("u", "v")}
    n3 = Buf((6,), torch.full((6,), 7, dtype=I32), I32)
    outs = {k: Buf(s) for k, s in (("dfake", (B, K)), ("dh_fake", (B, T, J)), ("dh_real", (B, T, J)), ("dm_real", (B, T, J)),
                                   ("dm_fake", (B, T, J)), ("dwr", (B,)), ("dwf", (B,)), ("dw", (Q, B)), ("dom", (Q,)))}
    need = L.lib.kccot_weighted_sinkhorn_loss_dw_workspace_bytes(B, K)
    ws, wsb = workspace(need)

    def lb(wr_=wr.ptr(), B_=B, eps_=1.0, dwr_=outs["dwr"].ptr(), dwf_=outs["dwf"].ptr(), wsb_=wsb, want=EINVAL):
        call(L, "kccot_weighted_sinkhorn_loss_bwd_dw_f32", g1.ptr(), ins["real"].ptr(), ins["fake"].ptr(), B_, K, 1.0, *feats, T, J,
             eps_, 7, wr_, wf.ptr(), C3.ptr(), h3["u"].ptr(), h3["v"].ptr(), n3.ptr(), outs["dfake"].ptr(), outs["dh_fake"].ptr(),
             outs["dh_real"].ptr(), outs["dm_real"].ptr(), outs["dm_fake"].ptr(), dwr_, dwf_, ws.ptr(), wsb_, None, want=want)

    for kw in ({"wr_": None}, {"B_": 0}, {"eps_": 0.0}, {"dwr_": None}, {"dwf_": None}):
        lb(**kw)
    lb(wsb_=need - 4, want=EWORKSPACE)
    lb(wsb_=L.lib.kccot_weighted_sinkhorn_loss_workspace_bytes(B, K), want=EWORKSPACE)
    assert ws.untouched()
    wq = Buf((Q, B), torch.full((Q, B), 1.0 / B))
    hq = {k: Buf((Q, 3, 7, B), torch.zeros(Q, 3, 7, B)) for k in ("u", "v")}
    nq = Buf((2, Q, 3), torch.full((2, Q, 3), 7, dtype=I32), I32)
    cost = Buf((Q, 3), torch.ones(Q, 3))
    need = L.lib.kccot_conditional_sinkhorn_loss_dw_workspace_bytes(B, K, Q)
    ws, wsb = workspace(need)

    def clb(w_=wq.ptr(), B_=B, Q_=Q, eps_=1.0, cost_=cost.ptr(), dw_=outs["dw"].ptr(), wsb_=wsb, want=EINVAL):
        call(L, "kccot_conditional_sinkhorn_loss_bwd_dw_f32", g1.ptr(), ins["real"].ptr(), ins["fake"].ptr(), B_, K, 1.0, *feats, T, J,
             eps_, 7, w_, None, Q_, C3.ptr(), hq["u"].ptr(), hq["v"].ptr(), nq.ptr(), outs["dfake"].ptr(), outs["dh_fake"].ptr(),
             outs["dh_real"].ptr(), outs["dm_real"].ptr(), outs["dm_fake"].ptr(), cost_, dw_, outs["dom"].ptr(), ws.ptr(), wsb_, None,
             want=want)

    for kw in ({"w_": None}, {"B_": 0}, {"Q_": 0}, {"eps_": 0.0}, {"cost_": None}, {"dw_": None}):
        clb(**kw)
    clb(wsb_=need - 4, want=EWORKSPACE)
    assert all(o.untouched() for o in outs.values()) and ws.untouched()
