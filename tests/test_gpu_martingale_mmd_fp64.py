"""csrc/martingale.hip held to float64: the martingale penalty p_M (forward and backward) and the single-GPU Gaussian-kernel
MMD, at the BASELINE shapes and at the edges of both kernels.  Inputs, case lists and seeds are those of
tests/test_oracle_martingale.py, which checks on the CPU what this module relies on (sign conditioning of every backward
case, the masked oracle, the fp32 emulation of the forward against the tolerances used here).

Martingale penalty
* forward: |p_M - ref| <= 1e-5 |ref| (the tolerance of test_gpu_abi_bounds.py::test_martingale), ref = fp64 oracle on the same
  fp32 values;
* backward: every element of dM against fp64 autograd of the oracle at GRAD_TOL of max |dM_ref|, upstream gradients 2.5, -1
  and 0 (exactly 0 out);
* near_martingale (the state the trainer drives towards: s is what rounding leaves), forward only, p_M alone, against the
  derived bound  lam sc sum_{t,q} (B + 8) 2^-24 (1/B) sum_b |N_std[b,t,q]|  (test_oracle_martingale.near_bound);
* dead_columns: std = 0 -- the documented convention (the path through std contributes 0 there) against
  oracle.gan_utils_torch.martingale_pieces: finite everywhere, exactly 0 on the dead columns;
* time_constant: p_M == 0 and dM == 0 exactly;
* shape edges through the C ABI on guarded buffers, the largest accepted LDS request (65536 bytes) included, and the first
  refused shape (KCCOT_EUNSUPPORTED, nothing launched).

RBF-MMD: K3 per entry at rtol 2e-5 / atol 1e-7, mmd_out at 16 2^-24 absolute (each K <= 1 carries at most ~3 2^-24: the fp32
argument costs a e^-a 2^-24 <= 2^-24 / e, expf the rest; four means enter the estimate, then one fp32 rounding), gD3 at 2e-5 of
max |ref|; B = 64 .. 512 and 257, gamma in three regimes (mid, saturating: K3 == identity pattern and mmd_out == 2 / B
exactly, flat: K ~ 1 and the estimate is a cancellation of means near 1 -- the absolute bound is the meaningful one).  The
kernel states that its sums are fp64: mmd_out must be the fp64 estimate of its OWN fp32 entries rounded once
(2^-24 relative + 1e-12 for the order of the fp64 sums), which an fp32 accumulator misses by orders of magnitude.

Largest errors measured on an MI355X (each test prints its figures, -s), kernels of commit ee94232 (this module changes none):
  p_M forward          1.72e-7 relative (the CPU emulation of the fp32 order: 1.82e-7 on the same cases; tolerance 1e-5)
  dM                   2.78e-7 of max |dM_ref| at the BASELINE shapes, 6.29e-7 at (2,2044,8)          (GRAD_TOL 2.5e-5)
  near_martingale      |p_M - ref| 1.5e-7 at most, 0.1 % of the derived bound; p_M agrees with the emulation's in all 7 digits printed
  K3                   4.3e-8 absolute;  gD3 1.37e-7 of max |ref|                                      (2e-5)
  mmd_out              1.26e-9 absolute = 0.02 x 2^-24 (bound 16 x 2^-24); 4.2e-10 from the fp64 estimate of its own entries
"""
import numpy as np
import pytest
import torch

import abi_guard as ag
import test_oracle_martingale as C
from test_gpu_abi_bounds import GRAD_TOL, close, guarded_call

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
FWD_RTOL = C.FWD_RTOL
MMD_ATOL = 16 * C.U24


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def G():
    from kccotgan_amd import gan_utils
    return gan_utils


def _dev(M32):
    return torch.from_numpy(np.ascontiguousarray(M32)).to(DEV)


def _public(G, M, lam, sc, upstream=None):
    """p_M (and dM) through the public function; M: device tensor."""
    M = M.detach().requires_grad_(upstream is not None)
    pm = G.scale_invariante_martingale_regularization(M, lam, sc)
    if upstream is None:
        return pm.detach(), None
    pm.backward(torch.tensor(float(upstream), device=DEV))
    torch.cuda.synchronize()
    return pm.detach(), M.grad


def _check_fwd(tag, pm, ref):
    err = abs(float(pm) - ref) / abs(ref)
    print("%s: p_M %.9g fp64 %.9g rel %.2e" % (tag, float(pm), ref, err))
    assert err <= FWD_RTOL, (tag, float(pm), ref)
    return err


def _check_bwd(tag, dM, ref, upstream):
    dM = dM.detach().cpu().double().numpy()
    assert np.isfinite(dM).all(), tag
    if upstream == 0.0:
        assert not dM.any(), (tag, "an upstream gradient of 0 must give exactly 0")
        return 0.0
    err = float(np.abs(dM - ref).max()) / float(np.abs(ref).max())
    print("%s upstream %g: max |dM - ref| / max |ref| = %.2e" % (tag, upstream, err))
    assert err <= GRAD_TOL, tag
    return err


# ---------------------------------------------------------------- martingale penalty
@pytest.mark.parametrize("kind", C.BASELINE_GENS)
@pytest.mark.parametrize("shape", C.BASELINE_SHAPES)
def test_martingale_baseline_shapes_against_fp64(G, shape, kind):
    M32 = C.generate(kind, shape, C.seed_of(kind, shape))
    M = _dev(M32)
    worst = [0.0, 0.0]
    for lam, sc in C.LAM_SC:
        tag = "%s %s lam %g sc %.4g" % (kind, shape, lam, sc)
        for up in C.UPSTREAM:
            ref, _, _, _, gref = C.reference(M32, lam, sc, upstream=up, masked=False)
            pm, dM = _public(G, M, lam, sc, up)
            worst[0] = max(worst[0], _check_fwd(tag, pm, ref))
            worst[1] = max(worst[1], _check_bwd(tag, dM, gref, up))
    print("WORST %s %s: forward %.2e backward %.2e" % (kind, shape, *worst))


@pytest.mark.parametrize("shape", C.NEAR_SHAPES)
def test_martingale_near_martingale_within_the_derived_bound(G, shape):
    M32 = C.generate("near_martingale", shape, 0)
    for lam, sc in C.LAM_SC:
        ref, _, _, mean_abs, _ = C.reference(M32, lam, sc)
        bound = C.near_bound(mean_abs, shape[0], lam, sc)
        pm, _ = _public(G, _dev(M32), lam, sc)
        print("near_martingale %s lam %g sc %.4g: p_M %.6e fp64 %.6e |diff| %.3e bound %.3e (%.3f of it)"
              % (shape, lam, sc, float(pm), ref, abs(float(pm) - ref), bound, abs(float(pm) - ref) / bound))
        assert abs(float(pm) - ref) <= bound


@pytest.mark.parametrize("shape", C.DEAD_SHAPES)
def test_martingale_dead_columns_follow_the_documented_convention(G, shape):
    kind = "dead_columns"
    M32 = C.generate(kind, shape, C.seed_of(kind, shape))
    dead = C.dead_mask(kind, shape)
    for lam, sc in C.LAM_SC:
        tag = "%s %s lam %g sc %.4g" % (kind, shape, lam, sc)
        for up in C.UPSTREAM:
            ref, _, std, _, gref = C.reference(M32, lam, sc, upstream=up)
            assert ((std == 0) == dead).all() and not gref[:, :, dead].any()
            pm, dM = _public(G, _dev(M32), lam, sc, up)
            _check_fwd(tag, pm, ref)
            assert not bool(dM[:, :, torch.from_numpy(dead).to(DEV)].any()), (tag, "dM on a dead column")
            _check_bwd(tag, dM, gref, up)


@pytest.mark.parametrize("shape", C.CONST_SHAPES)
def test_martingale_time_constant_input_gives_exact_zeros(G, shape):
    M = _dev(C.generate("time_constant", shape, 0))
    for up in (2.5, -1.0):
        pm, dM = _public(G, M, 1.5, 0.3, up)
        assert float(pm) == 0 and not bool(dM.any())


@pytest.mark.parametrize("shape", C.EDGE_SHAPES)
def test_martingale_shape_edges_through_the_abi(L, shape):
    B, T, J = shape
    kind = C.EDGE_GEN.get(shape, "walk")
    M32 = C.generate(kind, shape, C.seed_of(kind, shape))
    if shape == (2, 2044, 8):
        assert (3 * J + (T - 1) * J + 16) * 4 == 65536
    for lam, sc in C.LAM_SC:
        tag = "%s %s lam %g sc %.4g" % (kind, shape, lam, sc)
        pm = guarded_call(L, "kccot_martingale_fwd_f32", ["@M", B, T, J, lam, sc, "@pm_out", None], {"M": _dev(M32)},
                          {"pm_out": ((1,), F32)})["pm_out"]
        for up in C.UPSTREAM:
            ref, _, _, _, gref = C.reference(M32, lam, sc, upstream=up)
            dM = guarded_call(L, "kccot_martingale_bwd_f32", ["@M", B, T, J, lam, sc, "@gpm", "@dM", None],
                              {"M": _dev(M32), "gpm": torch.tensor([up], device=DEV)}, {"dM": ((B, T, J), F32)})["dM"]
            if T == 1:
                assert ref == 0 and float(pm[0]) == 0 and not bool(dM.any()), tag
                continue
            _check_fwd(tag, pm[0], ref)
            _check_bwd(tag, dM, gref, up)


def test_martingale_beyond_the_lds_limit_is_refused_without_a_launch(L, G):
    B, T, J = C.TOO_LARGE
    assert (3 * J + (T - 1) * J + 16) * 4 == 65536 + 4 * J
    M = torch.rand(B, T, J, device=DEV)
    gM = ag.guarded_input("M", M)
    gpm, gdM = ag.guarded(4, "output", "pm_out"), ag.guarded(4 * B * T * J, "output", "dM")
    gg = ag.guarded_input("gpm", torch.tensor([2.5], device=DEV))
    assert L.lib.kccot_martingale_fwd_f32(gM.ptr, B, T, J, 1.0, 0.5, gpm.ptr, None) == L.EUNSUPPORTED
    assert b"too large" in L.lib.kccot_last_error()
    assert L.lib.kccot_martingale_bwd_f32(gM.ptr, B, T, J, 1.0, 0.5, gg.ptr, gdM.ptr, None) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(ag.unwritten(gpm.view(F32, (1,))).all()) and bool(ag.unwritten(gdM.view(F32, (B, T, J))).all())
    assert all(g.verify() is None for g in (gM, gpm, gdM, gg))
    with pytest.raises(NotImplementedError):
        G.scale_invariante_martingale_regularization(M, 1.0, 0.5)


def test_martingale_wrapper_converts_float64_and_strided_inputs(G):
    shape = (64, 30, 8)
    M32 = C.generate("walk", shape, 0)
    M = _dev(M32)
    pm, dM = _public(G, M, 1.0, 1.0 / 15.0, 2.5)
    views = {"float64": M.double(), "permuted": M.permute(1, 0, 2).contiguous().permute(1, 0, 2),
             "float64 permuted": M.double().permute(2, 1, 0).contiguous().permute(2, 1, 0)}
    assert not views["permuted"].is_contiguous() and not views["float64 permuted"].is_contiguous()
    for name, V in views.items():
        assert torch.equal(V.float(), M)
        pm2, dM2 = _public(G, V, 1.0, 1.0 / 15.0, 2.5)
        assert dM2.dtype == V.dtype and dM2.shape == V.shape
        assert ag.same_bits(pm2, pm) and ag.same_bits(dM2.float(), dM), name


@pytest.mark.parametrize("kind,shape", [("walk", (512, 48, 8)), ("near_martingale", (64, 30, 8)), ("uniform", (65, 9, 17))])
def test_martingale_is_deterministic(G, kind, shape):
    M = _dev(C.generate(kind, shape, C.seed_of(kind, shape)))
    pm, dM = _public(G, M, 1.0, 1.0 / 15.0, -1.0)
    for _ in range(3):
        pm2, dM2 = _public(G, M.clone(), 1.0, 1.0 / 15.0, -1.0)
        assert ag.same_bits(pm2, pm) and ag.same_bits(dM2, dM)


# ---------------------------------------------------------------- RBF-MMD
MMD_B = (64, 128, 256, 512, 257)
MMD_K = 960                            # features per sample: enough for the distances to concentrate as a video's do


def _videos(B, regime, seed):
    """BASELINE.md's inputs: real ~ U[0,1); fake = clip(real + 0.05 N(0,1), 0, 1) ("near") or independent U[0,1) ("far")."""
    rng = np.random.default_rng([seed, B])
    real = rng.random((B, MMD_K))
    fake = np.clip(real + 0.05 * rng.standard_normal((B, MMD_K)), 0, 1) if regime == "near" else rng.random((B, MMD_K))
    return real, fake


def _dist3(B, regime, seed):
    """[3,B,B] = (xy, xx, yy) squared distances, built in fp64 and rounded to fp32; xx and yy have an exactly zero diagonal."""
    x, y = _videos(B, regime, seed)
    out = []
    for a, b in ((x, y), (x, x), (y, y)):
        D = np.maximum((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T, 0.0)
        if a is b:
            np.fill_diagonal(D, 0.0)
        out.append(D)
    return torch.from_numpy(np.stack(out).astype(np.float32))


def _off_diagonal(D3):
    """All of xy and the off-diagonal entries of xx and yy."""
    B = D3.shape[1]
    eye = torch.eye(B, dtype=torch.bool)
    return torch.cat([D3[0].reshape(-1), D3[1][~eye], D3[2][~eye]])


def _gamma(D3, regime):
    off = _off_diagonal(D3).double()
    if regime == "mid":
        return 1.0 / float(off.median())
    if regime == "saturating":
        return 110.0 / float(off.min())          # gamma D >= 110 > 104: expf(-104) is below half the smallest fp32 subnormal
    return 1e-4 / float(off.max())


def _mmd(L, D3, gamma, with_K3=True, stream=None):
    B = D3.shape[1]
    K3 = torch.empty_like(D3) if with_K3 else None
    m = torch.empty(1, device=DEV)
    rc = L.lib.kccot_rbf_mmd_f32(D3.data_ptr(), B, gamma, K3.data_ptr() if with_K3 else None, m.data_ptr(), stream)
    assert rc == 0, L.lib.kccot_last_error()
    return K3, m


@pytest.mark.parametrize("gamma_regime", ["mid", "saturating", "flat"])
@pytest.mark.parametrize("regime", ["near", "far"])
@pytest.mark.parametrize("B", MMD_B)
def test_rbf_mmd_against_fp64(L, B, regime, gamma_regime):
    D3 = _dist3(B, regime, B)
    gamma = float(np.float32(_gamma(D3, gamma_regime)))          # the value the ABI's `float gamma` receives
    fwd = guarded_call(L, "kccot_rbf_mmd_f32", ["@D3", B, gamma, "@K3_out", "@mmd_out", None], {"D3": D3.to(DEV)},
                       {"K3_out": ((3, B, B), F32), "mmd_out": ((1,), F32)})
    K3, got = fwd["K3_out"].cpu(), float(fwd["mmd_out"][0])
    Dd = D3.double().requires_grad_(True)
    K = torch.exp(-gamma * Dd)
    m = K[1].mean() + K[2].mean() - 2 * K[0].mean()
    ref = float(m.detach())
    own = K3.double()
    own = float(own[1].mean() + own[2].mean() - 2 * own[0].mean())
    kerr = float((K3.double() - K.detach()).abs().max())
    print("B %d %s %s gamma %.4g: mmd %.9g fp64 %.9g |diff| %.2e (%.2f x 2^-24); of its own entries %.2e; max |dK| %.2e"
          % (B, regime, gamma_regime, gamma, got, ref, abs(got - ref), abs(got - ref) / C.U24, abs(got - own), kerr))
    close(K3, K, 0, "K3", rtol=2e-5, atol=1e-7)
    assert abs(got - ref) <= MMD_ATOL
    assert abs(got - own) <= C.U24 * abs(own) + 1e-12, "mmd_out is not the fp64 estimate of the kernel's own entries"
    if gamma_regime == "saturating":
        eye = torch.eye(B)
        assert float(gamma * _off_diagonal(D3).min()) > 104
        assert torch.equal(K3, torch.stack([torch.zeros(B, B), eye, eye])), "saturated entries must be exactly 0, the diagonal 1"
        assert got == float(np.float32(2.0 / B))
    if gamma_regime == "flat":
        assert float(K3.min()) >= 1 - 1.001e-4
    (m * 3.0).backward()
    gD = guarded_call(L, "kccot_rbf_mmd_bwd_f32", ["@K3", B, gamma, "@gmmd", "@gD3", None],
                      {"K3": fwd["K3_out"], "gmmd": torch.tensor([3.0], device=DEV)}, {"gD3": ((3, B, B), F32)})["gD3"]
    gerr = float((gD.cpu().double() - Dd.grad).abs().max()) / float(Dd.grad.abs().max())
    print("B %d %s %s: max |gD3 - ref| / max |ref| = %.2e" % (B, regime, gamma_regime, gerr))
    close(gD, Dd.grad, 2e-5, "gD3")
    # K3_out == NULL: the same scalar
    _, m0 = _mmd(L, D3.to(DEV), gamma, with_K3=False)
    torch.cuda.synchronize()
    assert ag.same_bits(m0, fwd["mmd_out"])


@pytest.mark.parametrize("B", MMD_B)
def test_rbf_sum_blocks_give_the_one_call_kernel_values(L, B):
    """include/kccot.h: KCCOT_COST_RBF_SUM evaluates the expression of kccot_rbf_mmd_f32, so equal distances give the same
    kernel values bit for bit -- here with each matrix of D3 as one [B,B] block, and the block sums reproduce mmd_out."""
    D3 = _dist3(B, "near", B).to(DEV)
    gamma = float(np.float32(_gamma(D3.cpu(), "mid")))
    K3, m = _mmd(L, D3, gamma)
    torch.cuda.synchronize()
    need = int(L.lib.kccot_pairwise_cost_workspace_bytes(B, B, 1))
    sums = []
    for p in range(3):
        gC, gws = ag.guarded_input("C_out", D3[p].contiguous()), ag.guarded(need, "workspace", "ws")
        rc = L.lib.kccot_pairwise_cost_f32(None, None, B, B, 0, gamma, None, None, None, None, 0, 0, L.COST_RBF_SUM, gC.ptr,
                                           gws.ptr, gws.nbytes, None)
        assert rc == 0, L.lib.kccot_last_error()
        torch.cuda.synchronize()
        assert gC.verify() is None and gws.verify() is None
        assert ag.same_bits(gC.view(F32, (B, B)), K3[p]), "matrix %d" % p
        sums.append(float(gws.payload()[:8].view(F64)[0]))
    est = (sums[1] + sums[2] - 2.0 * sums[0]) / (B * B)
    assert abs(float(m[0]) - est) <= C.U24 * abs(est) + 1e-12


def test_rbf_mmd_graph_replay_gives_the_eager_bits(L):
    B = 256
    D3 = _dist3(B, "far", B).to(DEV)
    gamma = float(np.float32(_gamma(D3.cpu(), "mid")))
    K_eager, m_eager = _mmd(L, D3, gamma)
    torch.cuda.synchronize()
    K3, m = torch.empty_like(D3), torch.empty(1, device=DEV)
    call = lambda s: L.lib.kccot_rbf_mmd_f32(D3.data_ptr(), B, gamma, K3.data_ptr(), m.data_ptr(), s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up off the capture
        assert call(side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert call(torch.cuda.current_stream().cuda_stream) == 0
    for _ in range(2):
        K3.fill_(float("nan"))
        m.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert ag.same_bits(K3, K_eager) and ag.same_bits(m, m_eager)
