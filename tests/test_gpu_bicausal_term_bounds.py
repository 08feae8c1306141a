"""Bounds of kccot_pairwise_cost3_f32 with KCCOT_COST_BICAUSAL_TERM_ONLY (C3 is input and output), on the guarded buffers
of tests/abi_guard.py: at the sharded shapes (B = 128, 256, 512), at ragged tile edges, at k-chunk edges ((T-1) J around
256) and with every pointer 4 bytes off its alignment, the guard zones around C3 and the features stay intact, the
features are not written, C3 becomes exactly C3_in + the second causal terms (fp64 oracle), and every refused flag
combination leaves C3 untouched."""
import numpy as np
import pytest
import torch

import abi_guard as ag
from oracle import gan_utils_torch as ot

pytestmark = pytest.mark.gpu
F32 = torch.float32
FEATS = ("h_fake", "h_real", "m_real", "m_fake")


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


def _inputs(B, T, J, seed):
    g = torch.Generator().manual_seed(seed)
    f = {k: torch.rand(B, T, J, generator=g) for k in FEATS}
    C3 = torch.randn(3, B, B, generator=g) * 10.0
    return C3, f


def _call(L, gc3, gf, B, T, J, sc, flags, real=None, fake=None):
    rc = L.lib.kccot_pairwise_cost3_f32(real, fake, B, 0, sc, *(gf[k].ptr for k in FEATS), T, J, flags, gc3.ptr, None, 0, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("B,T,J,offset", [(1, 4, 3, 0), (7, 4, 3, 0), (8, 30, 8, 0), (64, 30, 8, 0), (65, 2, 5, 0),
                                          (128, 10, 8, 0), (129, 31, 9, 0), (256, 10, 8, 0), (512, 30, 8, 0), (3, 1, 4, 0),
                                          (33, 30, 8, 4), (128, 33, 8, 4)])
def test_term_only_writes_exactly_c3_and_adds_the_second_causal_terms(L, B, T, J, offset):
    sc = 1.0 / 15.0
    C3, f = _inputs(B, T, J, B * 31 + T)
    gc3 = ag.guarded_input("C3", C3.cuda(), offset)
    gf = {k: ag.guarded_input(k, v.cuda(), offset) for k, v in f.items()}
    snap = {k: g.payload().clone() for k, g in gf.items()}
    assert _call(L, gc3, gf, B, T, J, sc, L.COST_BICAUSAL_TERM_ONLY) == 0, L.lib.kccot_last_error()
    bad = [m for m in (g.verify() for g in [gc3] + list(gf.values())) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)
    for k, g in gf.items():
        assert torch.equal(g.payload(), snap[k]), "the call wrote its input %s" % k
    got = gc3.view(F32, (3, B, B)).cpu().double()
    d = {k: v.double() for k, v in f.items()}
    add = torch.stack([ot.causal_term(d["h_real"], d["m_fake"], sc), ot.causal_term(d["h_real"], d["m_real"], sc),
                       ot.causal_term(d["h_fake"], d["m_fake"], sc)])
    want = C3.double() + add
    tol = 1e-6 * max(float(want.abs().max()), 1.0)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=tol)
    # the same call on the same C3 gives the same bits (fixed order of the partial sums)
    gc3b = ag.guarded_input("C3", C3.cuda(), offset)
    assert _call(L, gc3b, gf, B, T, J, sc, L.COST_BICAUSAL_TERM_ONLY) == 0
    assert ag.same_bits(gc3b.view(F32, (3, B, B)), gc3.view(F32, (3, B, B)))


@pytest.mark.parametrize("other", ["COST_SAME", "COST_FORCE_DIRECT", "COST_FORCE_MFMA", "COST_PARTIAL_ONLY",
                                   "COST_GRAM_SUMS_ONLY", "COST_FROM_GRAM_SUMS"])
def test_refused_flag_combinations_leave_c3_untouched(L, other):
    B, T, J, K = 64, 30, 8, 512
    C3, f = _inputs(B, T, J, 5)
    gc3 = ag.guarded_input("C3", C3.cuda())
    gf = {k: ag.guarded_input(k, v.cuda()) for k, v in f.items()}
    vids = {k: ag.guarded_input(k, torch.rand(B, K).cuda()) for k in ("real", "fake")}
    before = gc3.payload().clone()
    rc = _call(L, gc3, gf, B, T, J, 0.5, L.COST_BICAUSAL_TERM_ONLY | getattr(L, other), vids["real"].ptr, vids["fake"].ptr)
    assert rc == L.EINVAL and b"no other flag" in L.lib.kccot_last_error()
    assert torch.equal(gc3.payload(), before) and gc3.verify() is None
    assert all(g.verify() is None for g in list(gf.values()) + list(vids.values()))
