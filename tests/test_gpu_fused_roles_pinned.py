"""sinkhorn_fused_roles with its plans pinned in front of the barriers (keep_in_regs, sinkhorn.hip) against the one-role
kernel, bit for bit, through the C ABI -- at the shapes where a pinned barrier can go wrong and that
tests/test_gpu_fused_roles.py does not already hold.  Compared: cost3, both halves of nits, loss and dC, option
sinkhorn_fused_roles = 1 against 0, in the three-problem form (kccot_sinkhorn_divergence_fused_f32) and the four-problem
form (the mixed loss on a given Cmix).

The pins sit on three paths of the sweep: the plan in front of the loop (row role, only if nits >= 1), the plan of the
column role in pass A and the plan of the row role in pass B, which is skipped in the last iteration (`it > 1`).  So:
  * L = 1: one sweep iteration, the prologue plan is the only one the row role evaluates;
  * a solve that stops early, nits < L, on the stop rule itself (Lmin = 1 with a threshold the error falls below within a
    few iterations) and at Lmin = 1 and 2 with a threshold nothing exceeds;
  * sinkhorn_shortcut = 1 on a problem that jumps (the sweep then runs over history rows the jump copied);
  * n = 64 and 33 (8 lanes per line, EPT 8), n = 32 and 7 (16 lanes per line, EPT 2 and 1: the pin of a single register);
  * a second launch on the same ticket word and the same output buffers gives the same bits."""
import pytest
import torch

from test_gpu_fused_roles import DEV, L, _both, _random_costs, _reset_flags, _seeded_costs  # noqa: F401  (L, _reset_flags: fixtures)

NS = [64, 33, 32, 7]


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n", NS)
def test_single_iteration_and_early_stops(L, n, nprob):
    """Random costs in [0, 30), eps = 1, every iteration executed.  The stop rule's error (sum |du|, fp32 oracle on these
    sizes) is above 11 after the first iteration and below 3.4 from the fourth on, at every n here: a threshold of 5 stops
    the solve after more than one and fewer than L iterations whatever the last bits are."""
    L.set_option("sinkhorn_shortcut", 0)
    C = _random_costs(nprob, n, 1000 * n + nprob)
    for Lit, Lmin, thresh, want in ((1, 1, 1e-2, 1), (100, 1, 1e30, 1), (100, 2, 1e30, 2), (100, 1, 5.0, None)):
        got = _both(L, C, Lit, Lmin, thresh, True, (n, nprob, Lit, Lmin, thresh))
        nits = got["nits"].tolist()
        assert got["executed"].tolist() == nits, (Lit, Lmin, thresh)
        if want is not None:
            assert nits == [want] * nprob, (Lit, Lmin, thresh, nits)
        else:
            assert all(1 < k < Lit for k in nits), (Lit, Lmin, thresh, nits)


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n", NS)
def test_shortcut_jump(L, n, nprob):
    """The seeded near matrices reach an fp32 two-cycle after a handful of iterations at every n here (CPU oracle), so with
    sinkhorn_shortcut = 1 and Lmin = L = 100 both roles take the jump: fewer iterations executed than counted."""
    L.set_option("sinkhorn_shortcut", 1)
    C = _seeded_costs("near", nprob, n)
    got = _both(L, C, 100, 100, 1e-2, True, (n, nprob))
    assert got["nits"].tolist() == [100] * nprob and all(k < 100 for k in got["executed"].tolist()), (got["nits"], got["executed"])


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n", NS)
def test_second_launch_on_the_same_ticket(L, n, nprob):
    """Two consecutive launches of the role kernel on one ticket word (the last workgroup of the first resets it) and on the
    same output buffers: the second leaves the bits of the first."""
    from kccotgan_amd._lib import ptr
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_fused_roles", 1)
    assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, 7) == 1
    C = _random_costs(nprob, n, 2000 * n + nprob)
    cost = torch.full((nprob,), float("nan"), device=DEV)
    nits = torch.full((2 * nprob,), -7, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    dC = torch.full_like(C, float("nan"))
    runs = []
    for _ in range(2):
        if nprob == 3:
            rc = L.lib.kccot_sinkhorn_divergence_fused_f32(ptr(C), n, 1.0, 7, 7, 1e-2, ptr(cost), ptr(nits), ptr(loss), ptr(ticket),
                                                           ptr(dC), None)
        else:
            rc = L.lib.kccot_mixed_sinkhorn_loss_fwd_f32(None, None, n, 0, 0.0, *([None] * 6), 1, 1, 1.0, 7, 7, 1e-2,
                                                         L.MIXED_CMIX_GIVEN, ptr(C), None, None, ptr(dC), ptr(cost), ptr(nits),
                                                         ptr(loss), ptr(ticket), None, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, L.lib.kccot_last_error()
        assert int(ticket) == 0
        runs.append([x.clone() for x in (cost, nits, loss, dC)])
    assert not torch.isnan(runs[0][3]).any() and not torch.isnan(runs[0][2]).any() and runs[0][1].tolist() == [7] * (2 * nprob)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
