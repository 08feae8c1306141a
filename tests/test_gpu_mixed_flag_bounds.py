"""Bounds of the two flags of the batch-sharded mixed loss, on the guarded buffers of tests/abi_guard.py:

KCCOT_COST_CAUSAL_ADD (kccot_pairwise_cost_f32; C_out is input and output): at ragged tile edges, T = 1, J = 1, k-chunk
edges ((T-1) J around 256), the sharded shapes and with every pointer 4 bytes off its alignment, only C_out is written,
the guard zones and the features stay intact, C_out becomes C_in + the causal term (fp64 oracle), a second call gives the
same bits, and on zero blocks the result equals the single-GPU loss's Cmix of zero videos bit for bit.

KCCOT_MIXED_CMIX_GIVEN (kccot_mixed_sinkhorn_loss_fwd_f32; Cmix is input): on the fused and the history path, with the
documented workspace (none / kccot_sinkhorn_workspace_bytes(4, B)) and no videos or features, only the documented
outputs are written, Cmix is untouched, and cost4, nits, loss and dCmix_unit (fused) or the executed part of u_hist /
v_hist (history) are bit-identical to the normal call's on the same Cmix."""
import numpy as np
import pytest
import torch

import abi_guard as ag
from oracle import gan_utils_torch as ot

pytestmark = pytest.mark.gpu
F32 = torch.float32
SC = 1.0 / 15.0


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


def _add(L, gC, gh, gM, Bx, By, T, J, flags=None):
    rc = L.lib.kccot_pairwise_cost_f32(None, None, Bx, By, 0, SC, gh.ptr, gM.ptr, None, None, T, J,
                                       L.COST_CAUSAL_ADD if flags is None else flags, gC.ptr, None, 0, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("Bx,By,T,J,offset", [(1, 1, 4, 3, 0), (7, 9, 4, 3, 0), (16, 16, 30, 8, 0), (17, 33, 30, 8, 0),
                                              (32, 128, 30, 8, 0), (64, 512, 48, 8, 0), (3, 5, 1, 4, 0), (20, 40, 5, 1, 0),
                                              (33, 65, 33, 8, 4), (40, 80, 34, 8, 4), (128, 256, 10, 8, 0), (5, 300, 2, 1, 4)])
def test_causal_add_writes_exactly_c_out(L, Bx, By, T, J, offset):
    g = torch.Generator().manual_seed(Bx * 7 + By + T)
    h, M = torch.rand(Bx, T, J, generator=g), torch.rand(By, T, J, generator=g)
    C = torch.randn(Bx, By, generator=g) * 10.0
    gC = ag.guarded_input("C_out", C.cuda(), offset)
    gh, gM = ag.guarded_input("h", h.cuda(), offset), ag.guarded_input("M", M.cuda(), offset)
    snap = (gh.payload().clone(), gM.payload().clone())
    assert _add(L, gC, gh, gM, Bx, By, T, J) == 0, L.lib.kccot_last_error()
    bad = [m for m in (x.verify() for x in (gC, gh, gM)) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)
    assert torch.equal(gh.payload(), snap[0]) and torch.equal(gM.payload(), snap[1]), "the call wrote an input"
    got = gC.view(F32, (Bx, By)).cpu().double()
    want = C.double() + ot.causal_term(h.double(), M.double(), SC)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-6 * max(float(want.abs().max()), 1.0))
    if T == 1:
        assert ag.same_bits(gC.view(F32, (Bx, By)).cpu(), C), "T = 1: nothing may be added"
    gC2 = ag.guarded_input("C_out", C.cuda(), offset)
    assert _add(L, gC2, gh, gM, Bx, By, T, J) == 0
    assert ag.same_bits(gC2.view(F32, (Bx, By)), gC.view(F32, (Bx, By)))


@pytest.mark.parametrize("other", ["COST_SAME", "COST_FORCE_DIRECT", "COST_FORCE_MFMA", "COST_PARTIAL_ONLY",
                                   "COST_GRAM_SUMS_ONLY", "COST_FROM_GRAM_SUMS", "COST_BICAUSAL_TERM_ONLY", "MIXED_CMIX_GIVEN"])
def test_causal_add_refusals_leave_c_out_untouched(L, other):
    Bx, By, T, J = 16, 24, 6, 4
    gC = ag.guarded_input("C_out", torch.randn(Bx, By).cuda())
    gh, gM = ag.guarded_input("h", torch.rand(Bx, T, J).cuda()), ag.guarded_input("M", torch.rand(By, T, J).cuda())
    before = gC.payload().clone()
    assert _add(L, gC, gh, gM, Bx, By, T, J, L.COST_CAUSAL_ADD | getattr(L, other)) == L.EINVAL
    assert b"no other flag" in L.lib.kccot_last_error()
    assert torch.equal(gC.payload(), before) and all(x.verify() is None for x in (gC, gh, gM))


@pytest.mark.parametrize("B,T,J", [(64, 30, 8), (40, 5, 3), (17, 1, 4), (128, 34, 8)])
def test_causal_add_on_zero_blocks_equals_the_single_gpu_cmix_of_zero_videos(L, B, T, J):
    """With R = F = 0 the single-GPU Cmix holds its causal terms alone (mixed_cost_finalize); CAUSAL_ADD on four zero
    blocks must reproduce them bit for bit -- the summation order the row-block regime relies on."""
    from kccotgan_amd import gan_utils as G
    g = torch.Generator().manual_seed(B + T)
    names = ("h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p")
    f = {k: torch.rand(B, T, J, generator=g).cuda() for k in names}
    z = torch.zeros(B, 256, device="cuda")
    G.compute_mixed_sinkhorn_loss(z, z, z, z, SC, 0.8, 100, *(f[k] for k in names))
    ref = G.last_info["compute_mixed_sinkhorn_loss_Cmix"].clone()
    for k, (h, M) in enumerate((("h_fake", "m_real"), ("h_fake_p", "m_real_p"), ("h_real_p", "m_real"), ("h_fake_p", "m_fake"))):
        gC = ag.guarded_input("C_out", torch.zeros(B, B, device="cuda"))
        gh, gM = ag.guarded_input("h", f[h]), ag.guarded_input("M", f[M])
        assert _add(L, gC, gh, gM, B, B, T, J) == 0, L.lib.kccot_last_error()
        assert all(x.verify() is None for x in (gC, gh, gM))
        assert ag.same_bits(gC.view(F32, (B, B)), ref[k]), "block %d differs from the single-GPU Cmix" % k


def _full_call(L, B, K, T, J, fused, seed):
    """The normal forward on random stacked videos: (Cmix, cost4, nits, loss, dCmix_unit | (u_hist, v_hist))."""
    lib = L.lib
    g = torch.Generator().manual_seed(seed)
    R = torch.rand(2 * B, K, generator=g)
    F = (R + 0.05 * torch.randn(2 * B, K, generator=g)).clamp(0, 1)
    feats = [torch.rand(B, T, J, generator=g).cuda() for _ in range(6)]
    R, F = R.cuda(), F.cuda()
    Cmix, cost4, nits, loss = (torch.empty(4, B, B, device="cuda"), torch.empty(4, device="cuda"),
                               torch.empty(8, dtype=torch.int32, device="cuda"), torch.empty(1, device="cuda"))
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    dCu = torch.empty(4, B, B, device="cuda") if fused else None
    uh, vh = (None, None) if fused else (torch.empty(4, 100, B, device="cuda"), torch.empty(4, 100, B, device="cuda"))
    wsb = int(lib.kccot_mixed_sinkhorn_loss_workspace_bytes(B, K))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()
    rc = lib.kccot_mixed_sinkhorn_loss_fwd_f32(p(R), p(F), B, K, SC, *(p(t) for t in feats), T, J, 1.0, 100, 100, 0.01, 0,
                                               p(Cmix), p(uh), p(vh), p(dCu), p(cost4), p(nits), p(loss), p(ticket),
                                               p(ws), wsb, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.kccot_last_error()
    return Cmix, cost4, nits, loss, (dCu if fused else (uh, vh))


def _given_call(L, B, Cmix, fused, offset):
    lib = L.lib
    gC = ag.guarded_input("Cmix", Cmix, offset)
    out = {"cost4": ag.guarded(16, "output", "cost4_out", offset), "nits": ag.guarded(32, "output", "nits_out", offset),
           "loss": ag.guarded(4, "output", "loss_out", offset), "ticket": ag.guarded(4, "zero", "ticket", offset)}
    if fused:
        out["dCu"] = ag.guarded(16 * B * B, "output", "dCmix_unit", offset)
        ws, wsb = None, 0
    else:
        out["uh"] = ag.guarded(16 * 100 * B, "output", "u_hist", offset)
        out["vh"] = ag.guarded(16 * 100 * B, "output", "v_hist", offset)
        need = int(lib.kccot_sinkhorn_workspace_bytes(4, B))
        ws = ag.guarded(need, "workspace", "ws") if need else None
        wsb = need
    p = lambda k: out[k].ptr if k in out else None
    before = gC.payload().clone()
    rc = lib.kccot_mixed_sinkhorn_loss_fwd_f32(None, None, B, 0, 0.0, *([None] * 6), 1, 1, 1.0, 100, 100, 0.01,
                                               L.MIXED_CMIX_GIVEN, gC.ptr, p("uh"), p("vh"), p("dCu"), p("cost4"), p("nits"),
                                               p("loss"), p("ticket"), ws.ptr if ws else None, wsb, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.kccot_last_error()
    bad = [m for m in (x.verify() for x in [gC] + list(out.values()) + ([ws] if ws else [])) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)
    assert torch.equal(gC.payload(), before), "CMIX_GIVEN wrote its input Cmix"
    assert int(out["ticket"].view(torch.int32, (1,))[0]) == 0, "the ticket must be left zero"
    return out


@pytest.mark.parametrize("B,fused,offset", [(8, True, 0), (40, True, 4), (64, True, 0), (8, False, 0), (64, False, 4),
                                            (65, False, 0), (192, False, 0), (256, False, 4)])
def test_cmix_given_equals_the_normal_call_on_the_same_cmix(L, B, fused, offset):
    if fused:
        assert L.lib.kccot_sinkhorn_fused_eligible(B, 100)
    Cmix, cost4, nits, loss, state = _full_call(L, B, 256, 6, 4, fused, B * 3 + fused)
    outs = [_given_call(L, B, Cmix, fused, offset) for _ in range(2)]        # the second call: the same bits
    for out in outs:
        assert ag.same_bits(out["cost4"].view(F32, (4,)), cost4)
        assert ag.same_bits(out["nits"].view(torch.int32, (8,)), nits)
        assert ag.same_bits(out["loss"].view(F32, (1,)), loss)
        if fused:
            assert ag.same_bits(out["dCu"].view(F32, (4, B, B)), state)
        else:
            uh, vh = state
            gu, gv = out["uh"].view(F32, (4, 100, B)), out["vh"].view(F32, (4, 100, B))
            for p in range(4):
                # the executed iterations' rows as the normal call's; none at or past the reference's count (in between:
                # the iterations the exact periodic-state shortcut skipped, which the solver may fill in)
                n, n_ref = int(nits[4 + p]), int(nits[p])
                assert 0 < n <= n_ref <= 100
                assert ag.same_bits(gu[p, :n], uh[p, :n]) and ag.same_bits(gv[p, :n], vh[p, :n]), p
                assert bool(ag.unwritten(gu[p, n_ref:]).all()) and bool(ag.unwritten(gv[p, n_ref:]).all()), p
