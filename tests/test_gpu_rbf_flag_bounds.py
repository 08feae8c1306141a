"""KCCOT_COST_RBF_SUM (kccot_pairwise_cost_f32; C_out is input and output, the block's fp64 sum goes to ws[0]) on the guarded
buffers of tests/abi_guard.py.

Entries: against fp64 exp(-gamma D) of the same fp32 D.  expf on this hardware is not correctly rounded; the bound is 2 ulp
of fp32, and no more than the parent's one-workgroup kernel (kccot_rbf_mmd_f32) shows on the same D -- the new kernel
evaluates the same expression, so its entries must equal the parent's bit for bit (each test prints both distances).
Sum: 1e-12 relative of the fp64 sum of the kernel's own fp32 entries.  Bounds: nothing is written outside C_out and the
first 8 (1 + ceil(Bx / 4) ceil(By / 64)) bytes of a workspace of exactly kccot_pairwise_cost_workspace_bytes(Bx, By, 1)
bytes.  Two launches and a graph replay give identical bits.  Row blocks summed over all row blocks reproduce
kccot_rbf_mmd_f32's scalar on the full D3 within the bound tests/test_gpu_abi_bounds.py::test_rbf_mmd applies to it."""
import math

import numpy as np
import pytest
import torch

import abi_guard as ag

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
SHAPES = [(16, 16), (5, 37), (64, 64), (32, 256), (64, 512), (1, 1)]


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


def _need(L, Bx, By):
    return int(L.lib.kccot_pairwise_cost_workspace_bytes(Bx, By, 1))


def _call(L, gC, gws, Bx, By, gamma, flags=None, wsb=None, stream=None):
    return L.lib.kccot_pairwise_cost_f32(None, None, Bx, By, 0, gamma, None, None, None, None, 0, 0,
                                         L.COST_RBF_SUM if flags is None else flags, gC.ptr, gws.ptr,
                                         gws.nbytes if wsb is None else wsb, stream)


def _dist(Bx, By, seed, Kf=24):
    """A block of squared distances between random points, fp32, as the cost kernels would leave it (zeros included when
    the block is square: its diagonal)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(Bx, Kf, generator=g)
    y = x[:By] if Bx == By else torch.rand(By, Kf, generator=g)
    return ((x[:, None, :].double() - y[None, :, :].double()) ** 2).sum(-1).float().contiguous()


def _ulps(k32, k64):
    """Distance of fp32 values from fp64 ones in units of the fp32 spacing at the exact value."""
    k32, k64 = k32.double().numpy(), k64.numpy()
    return float(np.max(np.abs(k32 - k64) / np.spacing(np.abs(k64).astype(np.float32)).astype(np.float64)))


def _parent_entries(L, D, gamma):
    """exp(-gamma D) by the parent's kernel (kccot_rbf_mmd_f32 walks [3,B,B] as a flat array): the entries of D embedded in
    a zero-padded [3,n,n]."""
    n = int(math.ceil(math.sqrt(D.numel() / 3.0)))
    D3 = torch.zeros(3 * n * n, device="cuda")
    D3[:D.numel()] = D.reshape(-1).cuda()
    K3, m = torch.empty_like(D3), torch.empty(1, device="cuda")
    assert L.lib.kccot_rbf_mmd_f32(D3.data_ptr(), n, gamma, K3.data_ptr(), m.data_ptr(), None) == 0, L.lib.kccot_last_error()
    torch.cuda.synchronize()
    return K3[:D.numel()].reshape(D.shape).cpu()


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("Bx,By", SHAPES + [(3, 65), (7, 128), (130, 4)])
def test_rbf_sum_entries_sum_and_bounds(L, Bx, By, offset):
    gamma = 1.0 / 6.0
    D = _dist(Bx, By, Bx * 131 + By)
    need = _need(L, Bx, By)
    tiles = ((Bx + 3) // 4) * ((By + 63) // 64)
    span = 8 * (1 + tiles)
    assert span <= need
    gC = ag.guarded_input("C_out", D.cuda(), offset)               # offset 4: the scalar path (rows not 16-byte aligned)
    gws = ag.guarded(need, "workspace", "ws")
    assert _call(L, gC, gws, Bx, By, gamma) == 0, L.lib.kccot_last_error()
    torch.cuda.synchronize()
    bad = [m for m in (x.verify() for x in (gC, gws)) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)
    rest = gws.payload()[span:].view(torch.int32)
    assert bool((rest == ag._s32(ag.GUARD_WORD)).all()), "the call wrote the workspace behind its stated span"
    got = gC.view(F32, (Bx, By)).cpu()
    want = torch.exp(-gamma * D.double())
    parent = _parent_entries(L, D, gamma)
    u_new, u_parent = _ulps(got, want), _ulps(parent, want)
    print("[%d,%d] offset %d: entries %.3f ulp from fp64 (parent's kernel %.3f ulp)" % (Bx, By, offset, u_new, u_parent))
    assert u_new <= 2.0 and u_new <= u_parent
    assert ag.same_bits(got, parent), "the entries differ from kccot_rbf_mmd_f32's on the same distances"
    s = float(gws.payload()[:8].view(F64)[0])
    own = math.fsum(got.double().reshape(-1).tolist())
    print("[%d,%d] offset %d: sum %.17g, fp64 sum of its entries %.17g, rel %.2e" % (Bx, By, offset, s, own, abs(s - own) / own))
    assert abs(s - own) <= 1e-12 * own
    # a second launch: the same bits, entries and sum
    gC2, gws2 = ag.guarded_input("C_out", D.cuda(), offset), ag.guarded(need, "workspace", "ws")
    assert _call(L, gC2, gws2, Bx, By, gamma) == 0
    torch.cuda.synchronize()
    assert ag.same_bits(gC2.view(F32, (Bx, By)), gC.view(F32, (Bx, By)))
    assert ag.same_bits(gws2.payload()[:8].view(F64), gws.payload()[:8].view(F64))


@pytest.mark.parametrize("Bx,By", [(64, 512), (5, 37)])
def test_rbf_sum_graph_replay_gives_the_eager_bits(L, Bx, By):
    gamma = 0.125
    D = _dist(Bx, By, 7 * Bx + By).cuda()
    need = _need(L, Bx, By)
    gC, gws = ag.guarded_input("C_out", D), ag.guarded(need, "workspace", "ws")
    assert _call(L, gC, gws, Bx, By, gamma) == 0
    torch.cuda.synchronize()
    eager_K, eager_s = gC.view(F32, (Bx, By)).clone(), gws.payload()[:8].view(F64).clone()
    gC2, gws2 = ag.guarded_input("C_out", D), ag.guarded(need, "workspace", "ws")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up off the capture
        assert _call(L, gC2, gws2, Bx, By, gamma, stream=side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _call(L, gC2, gws2, Bx, By, gamma, stream=torch.cuda.current_stream().cuda_stream) == 0
    for _ in range(2):
        gC2.view(F32, (Bx, By)).copy_(D)                 # the call works in place: the distances go back in first
        gws2.fill(ag.GUARD_WORD)
        graph.replay()
        torch.cuda.synchronize()
        assert ag.same_bits(gC2.view(F32, (Bx, By)), eager_K) and ag.same_bits(gws2.payload()[:8].view(F64), eager_s)
    assert gC2.verify() is None and gws2.verify() is None


@pytest.mark.parametrize("B,rows,gamma", [(64, 16, 0.02), (128, 32, 0.01), (65, 13, 0.05)])
def test_row_blocks_reproduce_the_one_call_scalar(L, B, rows, gamma):
    """kccot_rbf_mmd_f32 on the full D3 against the flagged call on every [rows, B] block of it: the same kernel values,
    and (Sxx + Syy - 2 Sxy) / B^2 within the bound tests/test_gpu_abi_bounds.py::test_rbf_mmd applies to the scalar."""
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 9, generator=g)
    y = x + 0.3 * torch.rand(B, 9, generator=g)
    D3 = torch.stack([((a[:, None] - b[None]) ** 2).sum(-1) for a, b in ((x, y), (x, x), (y, y))]).float().cuda()
    K3, m = torch.empty_like(D3), torch.empty(1, device="cuda")
    assert L.lib.kccot_rbf_mmd_f32(D3.data_ptr(), B, gamma, K3.data_ptr(), m.data_ptr(), None) == 0
    torch.cuda.synchronize()
    sums = [0.0, 0.0, 0.0]
    for p in range(3):
        for r0 in range(0, B, rows):
            gC = ag.guarded_input("C_out", D3[p, r0:r0 + rows].contiguous())
            gws = ag.guarded(_need(L, rows, B), "workspace", "ws")
            assert _call(L, gC, gws, rows, B, gamma) == 0, L.lib.kccot_last_error()
            torch.cuda.synchronize()
            assert gC.verify() is None and gws.verify() is None
            assert ag.same_bits(gC.view(F32, (rows, B)), K3[p, r0:r0 + rows])
            sums[p] += float(gws.payload()[:8].view(F64)[0])
    got, want = (sums[1] + sums[2] - 2.0 * sums[0]) / (B * B), float(m[0])
    Kd = torch.exp(-gamma * D3.double().cpu())
    ref = float(Kd[1].mean() + Kd[2].mean() - 2 * Kd[0].mean())
    print("B %d: row blocks %.9g, one call %.9g, fp64 %.9g" % (B, got, want, ref))
    assert abs(got - ref) < 1e-5 * max(abs(ref), 1e-3) and abs(got - want) < 1e-5 * max(abs(want), 1e-3)


@pytest.mark.parametrize("other", ["COST_SAME", "COST_FORCE_DIRECT", "COST_FORCE_MFMA", "COST_PARTIAL_ONLY", "COST_GRAM_SUMS_ONLY",
                                   "COST_FROM_GRAM_SUMS", "COST_BICAUSAL_TERM_ONLY", "COST_CAUSAL_ADD", "MIXED_CMIX_GIVEN"])
def test_rbf_sum_refusals_leave_the_buffers_untouched(L, other):
    Bx, By = 16, 24
    gC = ag.guarded_input("C_out", _dist(Bx, By, 3).cuda())
    gws = ag.guarded(_need(L, Bx, By), "workspace", "ws")
    before = (gC.payload().clone(), gws.payload().clone())
    assert _call(L, gC, gws, Bx, By, 0.5, L.COST_RBF_SUM | getattr(L, other)) == L.EINVAL
    assert b"no other flag" in L.lib.kccot_last_error()
    assert _call(L, gC, gws, Bx, By, 0.0) == L.EINVAL and _call(L, gC, gws, Bx, By, 0.5, wsb=gws.nbytes - 8) == L.EWORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(gC.payload(), before[0]) and torch.equal(gws.payload(), before[1])
    assert gC.verify() is None and gws.verify() is None
