"""The role-split fused solve + reverse sweep (sinkhorn_fused_roles, option "sinkhorn_fused_roles" = 1) against the one-role
kernel (sinkhorn_fused_reg, = 0), bit for bit, through the C ABI: kccot_sinkhorn_divergence_fused_f32 (three problems) and
the four-problem entry of the mixed loss (kccot_mixed_sinkhorn_loss_fwd_f32 on a given Cmix).  Compared: cost_out, both
halves of nits_out, loss_out, dC and the ticket left at zero.

Shapes -- the smallest at which each way of the split can go wrong: n = 64 (2 x 512 threads, the full workgroup); 33 and 40
(the role boundary at 320 threads, pad lines and pad columns in both roles); 16 (one entry per lane), 17 and 32 at 16 lanes
per line; 64 at 4 lanes per line; 64 and 33 (pad columns) at 16 lanes per line and 100 with sinkhorn_fused_max_n = 128, where two
roles do not fit 1024 threads and the one-role kernel must run under either setting."""
import os

import numpy as np
import pytest
import torch

import cases
from oracle import gan_utils_np as o

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (n, sinkhorn_lanes_per_line, sinkhorn_fused_max_n, the role kernel runs)
SHAPES = [(64, 0, 64, True), (33, 0, 64, True), (40, 0, 64, True), (16, 0, 64, True), (17, 0, 64, True), (32, 0, 64, True),
          (64, 4, 64, True), (64, 16, 64, False), (33, 16, 64, False), (100, 0, 128, False)]
IDS = ["n%d_lanes%d" % s[:2] for s in SHAPES]
# (L, Lmin, thresh): L = 1, 2, 7, 100 with Lmin = L, and an early stop after Lmin = 3
ITERS = [(1, 1, 1e-2), (2, 2, 1e-2), (7, 7, 1e-2), (100, 100, 1e-2), (100, 3, 1e30)]


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


def _random_costs(nprob, n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((nprob, n, n), generator=g) * 30).to(DEV)          # bench.py, time_sinkhorn


_seeded = {}


def _seeded_costs(regime, nprob, n):
    """The xy / xx / yy (/ bi-causal xy) cost matrices of the seeded near / far case, cut to n x n: the committed 64 x 64
    matrices of cfg2, or (n > 64) the oracle's matrices of the decimated 128-sample case."""
    if n <= 64:
        if regime not in _seeded:
            g = np.load(os.path.join(GOLDEN, "cfg2_s0_near.npz" if regime == "near" else "cfg2_s1_far.npz"))
            _seeded[regime] = np.stack([g[k] for k in ("C_xy", "C_xx", "C_yy", "C_bicausal")])
        C = _seeded[regime]
    else:
        if (regime, 128) not in _seeded:
            i = cases.gen_inputs("deci128", 0 if regime == "near" else 1, regime)
            r, f = o.flatten_video(i["real"]), o.flatten_video(i["fake"])
            _seeded[(regime, 128)] = np.stack([
                o.modified_cost(r, f, i["h_fake"], i["m_real"], cases.SC), o.modified_cost(r, r, i["h_real"], i["m_real"], cases.SC),
                o.modified_cost(f, f, i["h_fake"], i["m_fake"], cases.SC),
                o.bi_causal_modified_cost(r, f, i["h_fake"], i["m_real"], i["h_real"], i["m_fake"], cases.SC)])
        C = _seeded[(regime, 128)]
    return torch.from_numpy(np.ascontiguousarray(C[:nprob, :n, :n], dtype=np.float32)).to(DEV)


def _solve(L, C, Lit, Lmin, thresh):
    """One fused launch through the C ABI on 3 or 4 problems; every output starts poisoned."""
    from kccotgan_amd._lib import ptr
    nprob, n = C.shape[0], C.shape[1]
    cost = torch.full((nprob,), float("nan"), device=DEV)
    nits = torch.full((2 * nprob,), -7, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    dC = torch.full_like(C, float("nan"))
    if nprob == 3:
        rc = L.lib.kccot_sinkhorn_divergence_fused_f32(ptr(C), n, 1.0, Lit, Lmin, thresh, ptr(cost), ptr(nits), ptr(loss),
                                                       ptr(ticket), ptr(dC), None)
    else:
        rc = L.lib.kccot_mixed_sinkhorn_loss_fwd_f32(None, None, n, 0, 0.0, *([None] * 6), 1, 1, 1.0, Lit, Lmin, thresh,
                                                     L.MIXED_CMIX_GIVEN, ptr(C), None, None, ptr(dC), ptr(cost), ptr(nits),
                                                     ptr(loss), ptr(ticket), None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, L.lib.kccot_last_error()
    return dict(cost=cost, nits=nits[:nprob], executed=nits[nprob:], loss=loss, dC=dC, ticket=ticket)


def _both(L, C, Lit, Lmin, thresh, roles_run, what):
    """The same launch with the option on and off: the role kernel runs exactly where the table says, every output is
    written, and all of them are the same bits."""
    n = C.shape[1]
    with L.options(sinkhorn_fused_roles=1):
        assert L.lib.kccot_sinkhorn_fused_eligible(n, Lit) == 1, what
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, Lit) == int(roles_run), what
        on = _solve(L, C, Lit, Lmin, thresh)
    with L.options(sinkhorn_fused_roles=0):
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, Lit) == 0, what
        off = _solve(L, C, Lit, Lmin, thresh)
    for k in ("cost", "nits", "executed", "loss", "dC"):
        assert not torch.isnan(off[k].float()).any() and (off[k] != -7).all(), (what, k, "not written")
        # the same bits (torch.equal alone would let +0 / -0 through)
        assert torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), (what, k)
    assert int(on["ticket"]) == 0 and int(off["ticket"]) == 0, (what, "ticket")
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n,lanes,max_n,roles_run", SHAPES, ids=IDS)
def test_roles_equal_one_role_on_random_costs(L, n, lanes, max_n, roles_run, nprob):
    """Every iteration executed (sinkhorn_shortcut = 0) at L = 1, 2, 7, 100 and an early stop after three iterations."""
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_lanes_per_line", lanes)
    L.set_option("sinkhorn_fused_max_n", max_n)
    C = _random_costs(nprob, n, 100 * n + nprob)
    for Lit, Lmin, thresh in ITERS:
        got = _both(L, C, Lit, Lmin, thresh, roles_run, (Lit, Lmin, thresh))
        want = Lmin if thresh > 1 else Lit
        assert got["nits"].tolist() == [want] * nprob and got["executed"].tolist() == [want] * nprob, (Lit, Lmin, got["nits"])


def _first_period(uh, vh):
    """First iteration count k at which the state equals, bit for bit, the state p <= 4 iterations earlier."""
    for i in range(1, len(uh)):
        for p in range(1, 5):
            if i - p >= 0 and np.array_equal(uh[i], uh[i - p]) and np.array_equal(vh[i], vh[i - p]):
                return i + 1
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("regime", ["near", "far"])
@pytest.mark.parametrize("n,lanes,max_n,roles_run", SHAPES, ids=IDS)
def test_roles_equal_one_role_on_the_seeded_cases(L, n, lanes, max_n, roles_run, regime, nprob):
    """The seeded near / far matrices with the exact periodic-state shortcut off and on.  Both regimes reach an fp32 fixed
    point (or a two-cycle) well before L = 100 at n <= 64 -- checked on the CPU oracle, whose loop executes every
    iteration -- so with the shortcut on the jump path of both roles runs: the executed count is below L."""
    L.set_option("sinkhorn_lanes_per_line", lanes)
    L.set_option("sinkhorn_fused_max_n", max_n)
    C = _seeded_costs(regime, nprob, n)
    for shortcut in (0, 1):
        L.set_option("sinkhorn_shortcut", shortcut)
        for Lit, Lmin, thresh in ((100, 100, 1e-2), (100, 3, 1e-2), (7, 7, 1e-2)):
            got = _both(L, C, Lit, Lmin, thresh, roles_run, (shortcut, Lit, Lmin))
            if shortcut and n <= 64 and Lmin == 100:
                r = o.sinkhorn_from_cost(C[0].cpu().numpy(), 1.0, 100, 100, history=True)
                k = _first_period(r[5], r[6])
                assert k is not None and k + 2 < Lit - 1, k             # the oracle's state repeats: there is a jump to make
                assert int(got["executed"][0]) < Lit and int(got["nits"][0]) == r[1], (got["executed"], got["nits"], r[1])
            elif not shortcut:
                assert torch.equal(got["executed"], got["nits"])


def _loss_and_grads(t):
    from kccotgan_amd import gan_utils as G
    wrt = ("fake", "h_fake", "h_real", "m_real", "m_fake")
    loss = G.compute_sinkhorn_loss(t["real"], t["fake"], cases.SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"],
                                   t["m_fake"], video=True)
    assert G.last_info["compute_sinkhorn_loss_fused_sweep"] is True
    return [loss.detach().clone()] + [x.clone() for x in torch.autograd.grad(loss, [t[k] for k in wrt])]


@pytest.mark.gpu
def test_loss_and_graph_replay_with_roles_equal_the_one_role_kernel(L):
    """compute_sinkhorn_loss forward + backward at the `small` golden shape: the loss and all five gradients with the option on
    equal the option off, and a GraphedLossStep captured with the option on replays the eager result."""
    from kccotgan_amd.graph import GraphedLossStep
    inp = cases.gen_inputs("small", 0, "near")
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    for k in ("fake", "h_fake", "h_real", "m_real", "m_fake"):
        t[k].requires_grad_(True)
    with L.options(sinkhorn_fused_roles=0):
        off = _loss_and_grads(t)
    with L.options(sinkhorn_fused_roles=1):
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(16, 100) == 1
        on = _loss_and_grads(t)
        step = GraphedLossStep(t, cases.SC)
        loss, grads = step()
        torch.cuda.synchronize()
        replay = [loss] + [grads[k] for k in ("fake", "h_fake", "h_real", "m_real", "m_fake")]
    for a, b, c in zip(on, off, replay):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
