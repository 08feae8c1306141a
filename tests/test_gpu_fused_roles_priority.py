"""sinkhorn_fused_roles with the chain pass of either role at a raised wave priority (sweep_prio, sinkhorn.hip) against the
one-role kernel, bit for bit, through the C ABI.  The priority changes which wave the SIMD issues next and nothing that a
wave computes, so every output (three or four costs, the iteration counts reported and executed, the loss, dC) of option
sinkhorn_fused_roles = 1 must be the bytes of = 0.

Shapes: the smallest that reach each instance of the kernel -- n = 64 (<8,8>), n = 64 at 4 lanes per line (<16,4>), n = 33
(<8,8>, pad lines and columns in both roles), n = 32 (<2,16>) and n = 7 (<1,16>) -- each with three problems and with four
through the mixed entry point.  The s_setprio pairs sit in the sweep loop and in its peeled first iteration, so: L = 1 (the
peeled iteration alone), 2 (one trip of the loop), 100; an early stop; the shortcut on with a batch that jumps (the sweep
then leaves through the same exits after a shorter forward loop); a second launch on the same ticket; and a captured graph
replayed five times against the eager result."""
import pytest
import torch

import cases
from test_gpu_fused_roles import DEV, L, _both, _loss_and_grads, _random_costs, _reset_flags, _seeded_costs, _solve  # noqa: F401  (L, _reset_flags: fixtures)

# (n, sinkhorn_lanes_per_line)
SHAPES = [(64, 0), (64, 4), (33, 0), (32, 0), (7, 0)]
IDS = ["n%d_lanes%d" % s for s in SHAPES]
OUTPUTS = ("cost", "nits", "executed", "loss", "dC")


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n,lanes", SHAPES, ids=IDS)
def test_every_output_equals_the_one_role_kernel(L, n, lanes, nprob):
    """Random costs in [0, 30), every iteration executed: L = 1, 2, 100 and a stop after Lmin = 3 of 100."""
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_lanes_per_line", lanes)
    C = _random_costs(nprob, n, 3000 * n + 10 * lanes + nprob)
    for Lit, Lmin, thresh in ((1, 1, 1e-2), (2, 2, 1e-2), (100, 100, 1e-2), (100, 3, 1e30)):
        got = _both(L, C, Lit, Lmin, thresh, True, (n, lanes, nprob, Lit, Lmin))
        want = Lmin if thresh > 1 else Lit
        assert got["nits"].tolist() == [want] * nprob and got["executed"].tolist() == [want] * nprob, (Lit, Lmin, got["nits"])


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n,lanes", SHAPES, ids=IDS)
def test_shortcut_with_a_jump_equals_the_one_role_kernel(L, n, lanes, nprob):
    """The seeded near matrices reach an fp32 fixed point or two-cycle within a handful of iterations at n <= 64 (CPU oracle,
    tests/test_gpu_fused_roles.py), so with sinkhorn_shortcut = 1 and Lmin = L = 100 the solve jumps."""
    L.set_option("sinkhorn_shortcut", 1)
    L.set_option("sinkhorn_lanes_per_line", lanes)
    C = _seeded_costs("near", nprob, n)
    got = _both(L, C, 100, 100, 1e-2, True, (n, lanes, nprob))
    assert got["nits"].tolist() == [100] * nprob and all(k < 100 for k in got["executed"].tolist()), (got["nits"], got["executed"])


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n,lanes", SHAPES, ids=IDS)
def test_second_launch_on_the_same_ticket_equals_the_one_role_kernel(L, n, lanes, nprob):
    """Two launches of the role kernel, the second on the ticket word the first one's last workgroup reset: both give the
    bytes of the one-role kernel."""
    from kccotgan_amd._lib import ptr
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_lanes_per_line", lanes)
    C = _random_costs(nprob, n, 4000 * n + 10 * lanes + nprob)
    with L.options(sinkhorn_fused_roles=0):
        off = _solve(L, C, 7, 7, 1e-2)
    L.set_option("sinkhorn_fused_roles", 1)
    assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, 7) == 1
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for launch in range(2):
        cost = torch.full((nprob,), float("nan"), device=DEV)
        nits = torch.full((2 * nprob,), -7, dtype=torch.int32, device=DEV)
        loss = torch.full((1,), float("nan"), device=DEV)
        dC = torch.full_like(C, float("nan"))
        if nprob == 3:
            rc = L.lib.kccot_sinkhorn_divergence_fused_f32(ptr(C), n, 1.0, 7, 7, 1e-2, ptr(cost), ptr(nits), ptr(loss), ptr(ticket),
                                                           ptr(dC), None)
        else:
            rc = L.lib.kccot_mixed_sinkhorn_loss_fwd_f32(None, None, n, 0, 0.0, *([None] * 6), 1, 1, 1.0, 7, 7, 1e-2,
                                                         L.MIXED_CMIX_GIVEN, ptr(C), None, None, ptr(dC), ptr(cost), ptr(nits),
                                                         ptr(loss), ptr(ticket), None, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, L.lib.kccot_last_error()
        assert int(ticket) == 0, launch
        on = dict(cost=cost, nits=nits[:nprob], executed=nits[nprob:], loss=loss, dC=dC)
        for k in OUTPUTS:
            assert torch.equal(on[k].view(torch.int32), off[k].view(torch.int32)), (launch, k)


@pytest.mark.gpu
def test_five_graph_replays_equal_the_eager_one_role_result(L):
    """compute_sinkhorn_loss forward + backward at the `small` golden shape (n = 16): a GraphedLossStep captured with the role
    kernel on, replayed five times, gives each time the loss and the five gradients of the eager one-role run."""
    from kccotgan_amd.graph import GraphedLossStep
    inp = cases.gen_inputs("small", 0, "near")
    t = {k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}
    wrt = ("fake", "h_fake", "h_real", "m_real", "m_fake")
    for k in wrt:
        t[k].requires_grad_(True)
    with L.options(sinkhorn_fused_roles=0):
        off = _loss_and_grads(t)
    with L.options(sinkhorn_fused_roles=1):
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(16, 100) == 1
        step = GraphedLossStep(t, cases.SC)
        for replay in range(5):
            loss, grads = step()
            torch.cuda.synchronize()
            for a, b in zip([loss] + [grads[k] for k in wrt], off):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), replay
