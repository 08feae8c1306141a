"""The serial sections of the fused solve + reverse sweep (the stretch between its two loops and the one behind them:
cost hand-off in the tail, the cost formed from the prologue's registers, dC transposed through LDS) against the UNTOUCHED
two-launch path, bit for bit, through the C ABI.

Both fused bodies (sinkhorn_fused_roles, option "sinkhorn_fused_roles" = 1, and sinkhorn_fused_reg, = 0) carry the same
sections, so comparing them with each other would let a common mistake through; the reference here is the pair of register
kernels with the dual history in global memory: kccot_sinkhorn_divergence_fwd_f32 + kccot_sinkhorn_divergence_bwd_f32 on
three problems, kccot_sinkhorn_fwd_f32 + kccot_sinkhorn_bwd_f32 with the weights {+1, +1, -1, -1} on the four of the mixed
entry (loss = ((c0 + c1) - c2) - c3 in fp32, left to right).  dC of the fused kernels equals the two-kernel path at the same
lanes per line, so the reference runs at the lanes the fused kernel takes (8 above n = 32 unless the option says 4).

Compared: cost, nits reported and executed, loss, dC.  Every output buffer starts as NaN or -7, so a word nobody wrote shows;
the ticket must be left at zero.  Shapes (n, lanes): (64, 0) the headline, two full roles; (64, 4) 16 entries per lane; (33, 0)
pad lines and pad columns in the LDS tile at pitch 34; (32, 0) 16 lanes per line, two entries per lane; (7, 0) one entry per
lane, one wave per role.  Iterations: L = 1 (the history, 2 (L + 1) NS floats, is smaller than the n (n + 1) tile that aliases
it), L = 2, L = 100, an early stop after Lmin = 3, and the periodic-state shortcut on the seeded near batch, which jumps."""
import pytest
import torch

from test_gpu_fused_roles import DEV, L, _random_costs, _reset_flags, _seeded_costs, _solve  # noqa: F401 (fixtures)

# (n, sinkhorn_lanes_per_line)
SHAPES = [(64, 0), (64, 4), (33, 0), (32, 0), (7, 0)]
IDS = ["n%d_lanes%d" % s for s in SHAPES]
# (L, Lmin, thresh)
ITERS = [(1, 1, 1e-2), (2, 2, 1e-2), (100, 100, 1e-2), (100, 3, 1e30)]
KEYS = ("cost", "nits", "executed", "loss", "dC")

_ref_cache = {}


def _two_launch(L, C, lanes, Lit, Lmin, thresh, key):
    """The two-launch path on 3 or 4 problems, computed once per case and shared (kept unchanged by its users)."""
    if key in _ref_cache:
        return _ref_cache[key]
    from kccotgan_amd._lib import ptr
    nprob, n = C.shape[0], C.shape[1]
    uh = torch.full((nprob, max(Lit, 1), n), float("nan"), device=DEV)
    vh = torch.full_like(uh, float("nan"))
    cost = torch.full((nprob,), float("nan"), device=DEV)
    nits = torch.full((2 * nprob,), -7, dtype=torch.int32, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    dC = torch.full_like(C, float("nan"))
    ref_lanes = lanes if lanes else (8 if n > 32 else 0)
    with L.options(sinkhorn_fused=0, sinkhorn_lanes_per_line=ref_lanes):
        if nprob == 3:
            one = torch.ones(1, device=DEV)
            rc = L.lib.kccot_sinkhorn_divergence_fwd_f32(ptr(C), n, 1.0, Lit, Lmin, thresh, ptr(uh), ptr(vh), ptr(cost), ptr(nits),
                                                         ptr(loss), ptr(ticket), None, 0, None)
            assert rc == 0, L.lib.kccot_last_error()
            rc = L.lib.kccot_sinkhorn_divergence_bwd_f32(ptr(C), ptr(uh), ptr(vh), ptr(nits), n, 1.0, Lit, ptr(one), ptr(dC), None, 0,
                                                         None)
        else:
            w = torch.tensor([1.0, 1.0, -1.0, -1.0], device=DEV)
            rc = L.lib.kccot_sinkhorn_fwd_f32(ptr(C), 4, n, 1.0, Lit, Lmin, thresh, 0, ptr(uh), ptr(vh), ptr(cost), ptr(nits), None,
                                              None, 0, None)
            assert rc == 0, L.lib.kccot_last_error()
            rc = L.lib.kccot_sinkhorn_bwd_f32(ptr(C), ptr(uh), ptr(vh), ptr(nits), 4, n, 1.0, Lit, ptr(w), ptr(dC), None, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, L.lib.kccot_last_error()
    if nprob == 4:
        loss = (((cost[0] + cost[1]) - cost[2]) - cost[3]).reshape(1)
    ref = dict(cost=cost, nits=nits[:nprob], executed=nits[nprob:], loss=loss, dC=dC)
    for k in KEYS:
        assert not torch.isnan(ref[k].float()).any() and (ref[k] != -7).all(), (key, k, "reference not written")
    _ref_cache[key] = ref
    return ref


def _same_bits(got, ref, what):
    for k in KEYS:
        assert not torch.isnan(got[k].float()).any() and (got[k] != -7).all(), (what, k, "not written")
        assert torch.equal(got[k].view(torch.int32), ref[k].view(torch.int32)), (what, k)     # +0 / -0 told apart
    assert int(got["ticket"]) == 0, (what, "ticket")


def _check_both_bodies(L, C, lanes, Lit, Lmin, thresh, key):
    ref = _two_launch(L, C, lanes, Lit, Lmin, thresh, key)
    n = C.shape[1]
    for roles in (1, 0):
        with L.options(sinkhorn_fused_roles=roles, sinkhorn_lanes_per_line=lanes):
            assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, Lit) == roles, key
            _same_bits(_solve(L, C, Lit, Lmin, thresh), ref, (key, "roles=%d" % roles))
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n,lanes", SHAPES, ids=IDS)
def test_fused_bodies_equal_the_two_launch_path_on_random_costs(L, n, lanes, nprob):
    """Every iteration executed: L = 1, 2, 100 and a stop after Lmin = 3."""
    L.set_option("sinkhorn_shortcut", 0)
    C = _random_costs(nprob, n, 7000 + 10 * n + nprob)
    for Lit, Lmin, thresh in ITERS:
        ref = _check_both_bodies(L, C, lanes, Lit, Lmin, thresh, ("random", n, lanes, nprob, Lit, Lmin))
        want = Lmin if thresh > 1 else Lit
        assert ref["nits"].tolist() == [want] * nprob and ref["executed"].tolist() == [want] * nprob


@pytest.mark.gpu
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n,lanes", SHAPES, ids=IDS)
def test_fused_bodies_equal_the_two_launch_path_across_the_shortcut_jump(L, n, lanes, nprob):
    """The seeded near batch reaches an fp32 periodic state early: with the shortcut on, every form jumps (executed < L)."""
    L.set_option("sinkhorn_shortcut", 1)
    C = _seeded_costs("near", nprob, n)
    ref = _check_both_bodies(L, C, lanes, 100, 100, 1e-2, ("near", n, lanes, nprob))
    assert int(ref["executed"][0]) < 100 and int(ref["nits"][0]) == 100, (ref["executed"], ref["nits"])


@pytest.mark.gpu
@pytest.mark.parametrize("roles", [1, 0])
@pytest.mark.parametrize("nprob", [3, 4])
def test_two_launches_on_one_ticket_word(L, roles, nprob):
    """Back to back, the same ticket word, nothing reset in between: the last arriver of the first launch left it at zero, and
    the second launch combines its own three (four) costs."""
    from kccotgan_amd._lib import ptr
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_fused_roles", roles)
    n, Lit = 33, 2
    Cs = [_random_costs(nprob, n, 7100 + nprob), _random_costs(nprob, n, 7200 + nprob)]
    refs = [_two_launch(L, C, 0, Lit, Lit, 1e-2, ("ticket", k, nprob)) for k, C in enumerate(Cs)]
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    outs = []
    for C in Cs:
        o = dict(cost=torch.full((nprob,), float("nan"), device=DEV), nits=torch.full((2 * nprob,), -7, dtype=torch.int32, device=DEV),
                 loss=torch.full((1,), float("nan"), device=DEV), dC=torch.full_like(C, float("nan")))
        if nprob == 3:
            rc = L.lib.kccot_sinkhorn_divergence_fused_f32(ptr(C), n, 1.0, Lit, Lit, 1e-2, ptr(o["cost"]), ptr(o["nits"]), ptr(o["loss"]),
                                                           ptr(ticket), ptr(o["dC"]), None)
        else:
            rc = L.lib.kccot_mixed_sinkhorn_loss_fwd_f32(None, None, n, 0, 0.0, *([None] * 6), 1, 1, 1.0, Lit, Lit, 1e-2,
                                                         L.MIXED_CMIX_GIVEN, ptr(C), None, None, ptr(o["dC"]), ptr(o["cost"]),
                                                         ptr(o["nits"]), ptr(o["loss"]), ptr(ticket), None, 0, None)
        assert rc == 0, L.lib.kccot_last_error()
        outs.append(o)
    torch.cuda.synchronize()
    for k, (o, ref) in enumerate(zip(outs, refs)):
        got = dict(cost=o["cost"], nits=o["nits"][:nprob], executed=o["nits"][nprob:], loss=o["loss"], dC=o["dC"], ticket=ticket)
        _same_bits(got, ref, ("launch", k))


@pytest.mark.gpu
@pytest.mark.parametrize("roles", [1, 0])
def test_a_captured_graph_replayed_five_times(L, roles):
    """The fused launch captured once and replayed: every replay starts from poisoned outputs and the ticket the replay before
    it left, and writes the two-launch path's bits."""
    from kccotgan_amd._lib import ptr
    L.set_option("sinkhorn_shortcut", 0)
    L.set_option("sinkhorn_fused_roles", roles)
    n, Lit = 64, 2
    C = _random_costs(3, n, 7300)
    ref = _two_launch(L, C, 0, Lit, Lit, 1e-2, ("graph",))
    cost = torch.empty(3, device=DEV); nits = torch.empty(6, dtype=torch.int32, device=DEV)
    loss = torch.empty(1, device=DEV); dC = torch.empty_like(C)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    _solve(L, C, Lit, Lit, 1e-2)                                  # the library's one-time work happens outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = L.lib.kccot_sinkhorn_divergence_fused_f32(ptr(C), n, 1.0, Lit, Lit, 1e-2, ptr(cost), ptr(nits), ptr(loss), ptr(ticket),
                                                       ptr(dC), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.lib.kccot_last_error()
    for rep in range(5):
        cost.fill_(float("nan")); nits.fill_(-7); loss.fill_(float("nan")); dC.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _same_bits(dict(cost=cost, nits=nits[:3], executed=nits[3:], loss=loss, dC=dC, ticket=ticket), ref, ("replay", rep))
