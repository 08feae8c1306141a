"""The L1 ground cost on the GPU (KCCOT_COST_L1 of include/kccot.h on the direct-difference kernel of csrc/cost.hip; its adjoint,
include/kccot_l1.h, csrc/cost_l1_bwd.hip) against the fp64 oracle of tests/l1_oracle.py, through the C ABI with outputs and
workspace between guard zones, through the public functions, the loss and the trainer.

Tolerances: min(4 x the largest error measured on an MI355X over the grid, cap).  The caps are theorems about a float32
evaluation (tests/l1_oracle.py; tests/test_l1_cost_cpu.py shows a plain one stays inside):
    forward   |C - ref| / ref        cap (n + 2) 2^-24 = 1.13e-06 with n = 17 (l1_oracle.FWD_CHAIN)
    backward  |d - ref| / max|ref|   cap N 2^-24 max_r sum_c |sc W[r,c]| / max|ref| per case (l1_oracle.bwd_cap)
    loss      1e-4 relative (the bound of tests/test_gpu_parity.py); its gradients: cap max(2.5e-5, 4 x the distance of float32
              autograd of the same pipeline from the float64 one), the bound of that module's one-batch gradient tests
    measured  forward 1.929e-07   backward 7.084e-07 (the largest fraction of a case's cap: 0.36)
              loss 2.359e-07   loss gradients 5.222e-06 of max|grad| (float32 autograd of the oracle itself: up to 1.7e-06)
    allowed   forward 7.72e-07   backward min(2.83e-06, cap)   loss 1e-4   loss gradients min(2.09e-05, cap = 2.5e-05)
Elements at which every source ties with the target must be exactly 0 ("ties" inputs: values on a 1/8 grid, the context frames
of fake bit-equal to real's).  Each grid test prints its figures before it asserts."""
import pytest
import torch

import abi_guard as ag
import l1_oracle as lo
from oracle import gan_utils_torch as ot

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SC = lo.f32(1.0 / 15.0)
MEASURED = {"fwd": 1.929e-07, "bwd": 7.084e-07, "bwd_frac": 0.36, "loss": 2.359e-07, "lgrad": 5.222e-06}
TOL_FWD = min(4 * MEASURED["fwd"], lo.CAP_FWD)
TOL_BWD = 4 * MEASURED["bwd"]
TOL_LGRAD = 4 * MEASURED["lgrad"]
GRAD_TOL_FLOOR, GRAD_TOL_FACTOR = 2.5e-5, 4.0           # tests/test_gpu_parity.py
KINDS = ["noise", "ties"]
WRT = ["fake", "h_fake", "h_real", "m_real", "m_fake"]


def _lib():
    from kccotgan_amd import _lib
    return _lib


def _G():
    from kccotgan_amd import gan_utils
    return gan_utils


@pytest.fixture(scope="module")
def worst():
    w = {"fwd": 0.0, "bwd": 0.0, "bwd_frac": 0.0, "loss": 0.0, "lgrad": 0.0}
    yield w
    print("\nworst over the grid: forward |C - ref| / ref %.3e  backward |d - ref| / max|ref| %.3e (%.2f of its cap)  "
          "loss %.3e  loss gradients %.3e" % (w["fwd"], w["bwd"], w["bwd_frac"], w["loss"], w["lgrad"]))


def _done(rc, *bufs):
    torch.cuda.synchronize()
    assert rc == 0, _lib().lib.kccot_last_error()
    for b in bufs:
        assert b.verify() is None, b.verify()


def _inputs(named, offset=0):
    """Guarded copies of the inputs; returns (buffers, check) -- check() asserts that the call left them unchanged"""
    bufs = {k: ag.guarded_input(k, t.contiguous(), 4 * offset if k in ("x", "y") else 0) for k, t in named.items() if t is not None}

    def check():
        for k, b in bufs.items():
            assert torch.equal(b.view(torch.float32, tuple(named[k].shape)), named[k]), k + " changed"
    return bufs, check


def _p(bufs, k):
    return bufs[k].ptr if k in bufs else None


def k_cost(x, y, feats=(), flags=0, offset=0):
    """kccot_pairwise_cost_f32 with KCCOT_COST_L1: feats = () or (h1, M1) or (h1, M1, h2, M2); x is y: pass y = None (SAME)"""
    L = _lib()
    same = y is None
    Bx, K = x.shape
    By = Bx if same else y.shape[0]
    f = list(feats) + [None] * (4 - len(feats))
    bufs, unchanged = _inputs(dict(x=x, y=None if same else y, h1=f[0], M1=f[1], h2=f[2], M2=f[3]), offset)
    nb = L.lib.kccot_pairwise_cost_workspace_bytes(Bx, By, K)
    out, ws = ag.guarded(Bx * By * 4, "output", "C_out"), ag.guarded(nb, "workspace", "ws")
    fl = L.COST_L1 | flags | (L.COST_SAME if same else 0)
    _done(L.lib.kccot_pairwise_cost_f32(bufs["x"].ptr, bufs["x" if same else "y"].ptr, Bx, By, K, SC, _p(bufs, "h1"), _p(bufs, "M1"),
                                        _p(bufs, "h2"), _p(bufs, "M2"), lo.T, lo.J, fl, out.ptr, ws.ptr, nb, L.stream_of(x)),
          out, ws, *bufs.values())
    unchanged()
    C = out.view(torch.float32, (Bx, By))
    assert not bool(ag.unwritten(C).any()), "C_out not written everywhere"
    return C.clone()


def k_cost3(real, fake, feats):
    L = _lib()
    B, K = real.shape
    hf, hr, mr, mf = feats
    bufs, unchanged = _inputs(dict(real=real, fake=fake, hf=hf, hr=hr, mr=mr, mf=mf))
    nb = L.lib.kccot_pairwise_cost3_workspace_bytes(B, K)
    out, ws = ag.guarded(3 * B * B * 4, "output", "C3"), ag.guarded(nb, "workspace", "ws")
    _done(L.lib.kccot_pairwise_cost3_f32(bufs["real"].ptr, bufs["fake"].ptr, B, K, SC, bufs["hf"].ptr, bufs["hr"].ptr, bufs["mr"].ptr,
                                         bufs["mf"].ptr, lo.T, lo.J, L.COST_L1, out.ptr, ws.ptr, nb, L.stream_of(real)),
          out, ws, *bufs.values())
    unchanged()
    C3 = out.view(torch.float32, (3, B, B))
    assert not bool(ag.unwritten(C3).any())
    return C3.clone()


def k_bwd(g, x, y, want="xy", offset=0):
    """kccot_l1_cost_bwd_f32; y = None: SAME.  Returns (dx, dy), None where not asked for."""
    L = _lib()
    same = y is None
    Bx, K = x.shape
    By = Bx if same else y.shape[0]
    bufs, unchanged = _inputs(dict(g=g, x=x, y=None if same else y), offset)
    nb = L.lib.kccot_l1_cost_bwd_workspace_bytes(Bx, By)
    ws = ag.guarded(nb, "workspace", "ws")
    dx = ag.guarded(Bx * K * 4, "output", "dx", 4 * offset) if "x" in want else None
    dy = ag.guarded(By * K * 4, "output", "dy", 4 * offset) if "y" in want and not same else None
    _done(L.lib.kccot_l1_cost_bwd_f32(bufs["g"].ptr, bufs["x"].ptr, bufs["x" if same else "y"].ptr, Bx, By, K, SC,
                                      L.COST_SAME if same else 0, dx.ptr if dx else None, dy.ptr if dy else None, ws.ptr, nb,
                                      L.stream_of(x)), ws, *bufs.values(), *(b for b in (dx, dy) if b))
    unchanged()
    res = []
    for b, n in ((dx, Bx), (dy, By)):
        if b is None:
            res.append(None)
            continue
        v = b.view(torch.float32, (n, K))
        assert not bool(ag.unwritten(v).any()), b.name + " not written everywhere"
        res.append(v.clone())
    return res


def k_bwd3(g3, real, fake):
    L = _lib()
    B, K = real.shape
    bufs, unchanged = _inputs(dict(g3=g3, real=real, fake=fake))
    nb = L.lib.kccot_l1_cost3_bwd_workspace_bytes(B)
    ws, d = ag.guarded(nb, "workspace", "ws"), ag.guarded(B * K * 4, "output", "dfake")
    _done(L.lib.kccot_l1_cost3_bwd_f32(bufs["g3"].ptr, bufs["real"].ptr, bufs["fake"].ptr, B, K, SC, d.ptr, ws.ptr, nb,
                                       L.stream_of(real)), ws, d, *bufs.values())
    unchanged()
    v = d.view(torch.float32, (B, K))
    assert not bool(ag.unwritten(v).any()), "dfake not written everywhere"
    return v.clone()


def _data(kind, Bx, By, K, seed, offset=0):
    _lib()              # (kccotgan_amd before the first CUDA call: kccotgan_amd/__init__.py)
    return lo.rows(kind, Bx, By, K, seed, DEV, offset)


def _feats(Bx, By, seed):
    """h1 [Bx,T,J], M1 [By,T,J], h2, M2"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((n, lo.T, lo.J), generator=g) - 0.5).to(DEV) for n in (Bx, By, Bx, By)]


def _causal(h, M):
    """(the term in float64, sum_k |h| |dM|): oracle.gan_utils_torch.causal_term and the magnitude its float32 error scales with"""
    hd, Md = h.double().cpu(), M.double().cpu()
    dM = (Md[:, 1:] - Md[:, :-1]).abs()
    mag = (hd[:, :-1].abs()[:, None] * dM[None]).sum(-1).sum(-1) * SC
    return ot.causal_term(hd, Md, SC).to(DEV), mag.to(DEV)


def _check_forward(C, x, y, feats, worst, tag):
    """The L1 part against its relative bound; with causal terms, each adds the bound of a float32 dot product of (T - 1) J = 15
    terms with float32 differences dM -- (15 + 4) 2^-24 of sum |h| |dM| sc -- and the two additions 2^-24 of the sums so far."""
    ref = lo.l1_block(x.double(), y.double(), SC)
    if not feats:
        nz = ref > 0
        err = float(((C.double() - ref).abs()[nz] / ref[nz]).max()) if bool(nz.any()) else 0.0
        print("%s: |C - ref| / ref %.3e" % (tag, err))
        worst["fwd"] = max(worst["fwd"], err)
        assert err <= TOL_FWD, (tag, err)
        assert bool((C[~nz] == 0).all())
        return ref
    bound = TOL_FWD * ref
    total, mags = ref.clone(), ref.clone()
    for h, M in zip(feats[::2], feats[1::2]):
        term, mag = _causal(h, M)
        total, mags = total + term, mags + mag
        bound = bound + ((lo.T - 1) * lo.J + 4) * lo.U * mag
    bound = bound + 2 * lo.U * mags
    gap = float(((C.double() - total).abs() / bound).max())
    print("%s: %d causal term(s): |C - ref| at most %.2f of the bound" % (tag, len(feats) // 2, gap))
    assert gap <= 1.0, (tag, gap)
    return total


# ---- forward -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Bx,By,K,offset", lo.FWD_SHAPES, ids=lambda v: str(v))
def test_forward_blocks_meet_the_bound_with_and_without_causal_terms(Bx, By, K, offset, kind, worst):
    x, y = _data(kind, Bx, By, K, 21, offset)
    f = _feats(Bx, By, 22)
    plain = None
    for nterms in (0, 1, 2):
        C = k_cost(x, y, f[:2 * nterms], offset=offset)
        _check_forward(C, x, y, f[:2 * nterms], worst, "%s (%d,%d,%d)+%d" % (kind, Bx, By, K, offset))
        plain = C if plain is None else plain
    # FORCE_DIRECT is the path the flag takes anyway: the same bits
    assert ag.same_bits(k_cost(x, y, flags=_lib().COST_FORCE_DIRECT, offset=offset), plain)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,K", lo.SAME_SHAPES)
def test_same_problems_have_a_zero_diagonal_and_an_exactly_symmetric_l1_part(B, K, kind, worst):
    x, _ = _data(kind, B, B, K, 23)
    f = _feats(B, B, 24)
    C = k_cost(x, None)
    assert bool((C.diagonal() == 0).all()), "diagonal"
    assert ag.same_bits(C, C.t().contiguous()), "C != C.T"
    _check_forward(C, x, x, [], worst, "%s same (%d,%d)" % (kind, B, K))
    # the same block computed as an x-against-y problem (a copy of x): equal bits off the diagonal
    Cxy = k_cost(x, x.clone())
    off = ~torch.eye(B, dtype=torch.bool, device=DEV)
    assert torch.equal(C[off], Cxy[off])
    for nterms in (1, 2):
        Cc = k_cost(x, None, f[:2 * nterms])
        _check_forward(Cc, x, x, f[:2 * nterms], worst, "%s same (%d,%d)" % (kind, B, K))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", lo.COST3_B)
def test_cost3_equals_the_three_single_block_calls_bit_for_bit(B, kind, worst):
    _lib()
    real, fake = (v.reshape(B, -1) for v in lo.videos(kind, B, 25, DEV))
    hf, hr, mr, mf = feats = lo.features(B, 26, DEV)
    C3 = k_cost3(real, fake, feats)
    singles = (k_cost(real, fake, (hf, mr)), k_cost(real, None, (hr, mr)), k_cost(fake, None, (hf, mf)))
    for p, (name, one) in enumerate(zip(("xy", "xx", "yy"), singles)):
        assert ag.same_bits(C3[p], one), name
    _check_forward(C3[0], real, fake, (hf, mr), worst, "%s cost3 B=%d xy" % (kind, B))
    _check_forward(C3[2], fake, fake, (hf, mf), worst, "%s cost3 B=%d yy" % (kind, B))
    if kind == "ties":      # the context frames of sample i tie in C_xy[i,i]: only the predicted frames count
        ctx = lo.context_mask(B).to(DEV)
        ref = ((real.double() - fake.double()).abs() * ~ctx).sum(1) * SC + _causal(hf, mr)[0].diagonal()
        assert float((C3[0].diagonal().double() - ref).abs().max()) <= 1e-5


# ---- backward ----------------------------------------------------------------------------------------------------------------
# Shapes (l1_oracle.BWD_SHAPES / BWD_SAME / BWD_COST3): the forward's, plus the boundaries of l1_sign_apply's own tiling -- the row
# group of 8 target rows (7, 8, 9 rows: padded coefficient rows, a second group), the k tail of the 1024-column tile (K = 1023:
# scalar loads with a tail; 1024: one full tile; 1028 and 2052: a 4-column tail in a second and a third tile with vector loads),
# an unaligned base (K = 1028 one float into the storage: the scalar-load kernel on a shape the vector one would take) and
# source counts around the 4 rows in flight (3, 4, 5 and, in the loss form, 2 B = 10, 18).
def _check_adjoint(form, d, ref, g, all_tie, worst, tag):
    cap = lo.bwd_cap(form, g, ref, SC)
    err = float((d.double() - ref).abs().max()) / float(ref.abs().max())
    print("%s %s: |d - ref| / max|ref| %.3e (cap %.3e)" % (tag, form, err, cap))
    worst["bwd"], worst["bwd_frac"] = max(worst["bwd"], err), max(worst["bwd_frac"], err / cap)
    assert err <= min(TOL_BWD, cap), (tag, form, err, cap)
    # every element where all sources tie with the target: exactly 0, as the oracle
    assert bool((ref[all_tie] == 0).all()) and bool((d[all_tie] == 0).all()), (tag, form, "ties")


def _all_tie(a, S):
    return (a[:, None, :] == S[None, :, :]).all(1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("Bx,By,K,offset", lo.BWD_SHAPES, ids=lambda v: str(v))
def test_adjoint_dx_dy_and_both_meet_the_bound_and_are_deterministic(Bx, By, K, offset, kind, worst):
    x, y = _data(kind, Bx, By, K, 31, offset)
    g = lo.upstream((Bx, By), 32, DEV)
    dx, dy = k_bwd(g, x, y, "xy", offset)
    xd, yd, gd = x.double(), y.double(), g.double()
    tag = "%s (%d,%d,%d)+%d" % (kind, Bx, By, K, offset)
    if float((xd[:, None] - yd[None]).abs().max()) > 0:          # (a 1 x 1 x 1 problem may tie: then everything is 0)
        _check_adjoint("x", dx, lo.adjoint_x(gd, xd, yd, SC), g, _all_tie(x, y), worst, tag)
        _check_adjoint("y", dy, lo.adjoint_y(gd, xd, yd, SC), g, _all_tie(y, x), worst, tag)
    else:
        assert bool((dx == 0).all()) and bool((dy == 0).all())
    # one output at a time, and a second identical call: the same bits
    assert ag.same_bits(k_bwd(g, x, y, "x", offset)[0], dx) and ag.same_bits(k_bwd(g, x, y, "y", offset)[1], dy)
    again = k_bwd(g, x, y, "xy", offset)
    assert ag.same_bits(again[0], dx) and ag.same_bits(again[1], dy)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,K", lo.BWD_SAME)
def test_adjoint_of_a_same_problem(B, K, kind, worst):
    x, _ = _data(kind, B, B, K, 33)
    g = lo.upstream((B, B), 34, DEV)
    dx = k_bwd(g, x, None, "x")[0]
    _check_adjoint("same", dx, lo.adjoint_same(g.double(), x.double(), SC), g, _all_tie(x, x), worst, "%s same (%d,%d)" % (kind, B, K))
    assert ag.same_bits(k_bwd(g, x, None, "x")[0], dx)
    # against the two-operand call on a copy: dx + dy of an x-against-x problem is the same sum in another order
    ex, ey = k_bwd(g, x, x.clone(), "xy")
    assert float((ex.double() + ey.double() - dx.double()).abs().max()) <= 4 * lo.bwd_cap("same", g, dx.double(), SC) * float(dx.abs().max())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,K", lo.BWD_COST3)
def test_adjoint_of_the_loss_form(B, K, kind, worst):
    _lib()
    if K == 120:
        real, fake = (v.reshape(B, -1) for v in lo.videos(kind, B, 35, DEV))
        ctx = lo.context_mask(B).to(DEV)
    else:
        real, fake = _data(kind, B, B, K, 35)
        ctx = None
    g3 = lo.upstream((3, B, B), 36, DEV)
    d = k_bwd3(g3, real, fake)
    ref = lo.adjoint_fake(g3.double(), real.double(), fake.double(), SC)
    tie = _all_tie(fake, torch.cat((real, fake)))
    _check_adjoint("fake", d, ref, g3, tie, worst, "%s cost3 (%d,%d)" % (kind, B, K))
    assert ag.same_bits(k_bwd3(g3, real, fake), d)
    # gxx is not read
    g3b = g3.clone()
    g3b[1] = 7.0
    assert ag.same_bits(k_bwd3(g3b, real, fake), d)
    if kind == "ties" and ctx is not None:
        # the xy term alone at i = j: sample j's context frames tie with real[j] -- dfake[j, context] is exactly the oracle's 0
        only = torch.zeros_like(g3)
        only[0] = torch.diag(g3[0].diagonal())
        d1 = k_bwd3(only, real, fake)
        r1 = lo.adjoint_fake(only.double(), real.double(), fake.double(), SC)
        assert bool((r1[ctx] == 0).all()) and bool((d1[ctx] == 0).all())
        assert float((d1.double() - r1).abs().max()) <= lo.bwd_cap("fake", only, r1, SC) * float(r1.abs().max())
        assert int(ctx.sum()) > 0 and float(r1.abs().max()) > 0


# ---- the loss, end to end ----------------------------------------------------------------------------------------------------
def _oracle_loss(inp, dtype):
    """oracle L1 costs + causal terms -> sinkhorn_from_cost x 3 -> 2 xy - xx - yy, with autograd (CPU)"""
    d = {k: v.detach().cpu().to(dtype) for k, v in inp.items()}
    for k in WRT:
        d[k].requires_grad_(True)
    r, f = d["real"].reshape(d["real"].shape[0], -1), d["fake"].reshape(d["fake"].shape[0], -1)
    C = {"xy": lo.l1_block(r, f, SC) + ot.causal_term(d["h_fake"], d["m_real"], SC),
         "xx": lo.l1_block(r, r, SC) + ot.causal_term(d["h_real"], d["m_real"], SC),
         "yy": lo.l1_block(f, f, SC) + ot.causal_term(d["h_fake"], d["m_fake"], SC)}
    w = {k: ot.sinkhorn_from_cost(c, 1.0, 100)[0] for k, c in C.items()}
    loss = 2.0 * w["xy"] - w["xx"] - w["yy"]
    grads = torch.autograd.grad(loss, [d[k] for k in WRT])
    return loss.detach().double(), {k: float(v) for k, v in w.items()}, dict(zip(WRT, (g.double() for g in grads)))


def _loss_inputs(kind, B, seed):
    _lib()
    real, fake = lo.videos(kind, B, seed, DEV)
    hf, hr, mr, mf = lo.features(B, seed + 1, DEV)
    return dict(real=real, fake=fake, h_fake=hf, h_real=hr, m_real=mr, m_fake=mf)


def _gpu_loss(t, **kw):
    G = _G()
    t = dict(t)
    for k in WRT:
        t[k] = t[k].detach().clone().requires_grad_(True)
    loss = G.compute_sinkhorn_loss(t["real"], t["fake"], SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"], t["m_fake"], **kw)
    return loss, dict(zip(WRT, torch.autograd.grad(loss, [t[k] for k in WRT])))


@pytest.mark.parametrize("kind,B", [("noise", 8), ("ties", 8), ("noise", 64), ("noise", 130)])
def test_l1_loss_and_its_gradients_match_fp64_autograd(kind, B, worst):
    """B = 130 takes the n > 128 branch of _divergence_bwd"""
    G = _G()
    t = _loss_inputs(kind, B, 41)
    G.last_info.clear()
    loss, got = _gpu_loss(t, ground_cost="l1")
    assert sorted(G.last_info) == sorted("compute_sinkhorn_loss" + s for s in ("", "_executed", "_costs", "_C3", "_fused_sweep"))
    assert G.last_info["compute_sinkhorn_loss"].tolist() == [100, 100, 100]
    ref_loss, ref_w, ref = _oracle_loss(t, torch.float64)
    _, _, ref32 = _oracle_loss(t, torch.float32)
    scale = max(abs(float(ref_loss)), max(abs(v) for v in ref_w.values()))
    e_loss = abs(float(loss) - float(ref_loss)) / scale
    print("%s B=%d: loss %.6f (fp64 %.6f): %.3e relative" % (kind, B, float(loss), float(ref_loss), e_loss))
    worst["loss"] = max(worst["loss"], e_loss)
    assert e_loss <= 1e-4
    for k, w3 in zip(("xy", "xx", "yy"), G.last_info["compute_sinkhorn_loss_costs"].tolist()):
        assert abs(w3 - ref_w[k]) <= 1e-4 * scale, k
    for k in WRT:
        m = float(ref[k].abs().max())
        gap = float((ref32[k] - ref[k]).abs().max()) / m
        cap = max(GRAD_TOL_FLOOR, GRAD_TOL_FACTOR * gap)
        err = float((got[k].double().cpu() - ref[k]).abs().max()) / m
        print("%s B=%d d%s: %.3e of max|grad| (fp32 autograd of the oracle: %.3e, cap %.3e)" % (kind, B, k, err, gap, cap))
        worst["lgrad"] = max(worst["lgrad"], err)
        assert err <= min(TOL_LGRAD, cap), (k, err, cap)
    if kind == "ties":      # dfake on the context frames: the i = j tie of the xy term contributes nothing, as in the oracle
        assert tuple(got["fake"].shape) == tuple(t["fake"].shape)
    with pytest.raises(NotImplementedError, match="real"):
        G.compute_sinkhorn_loss(t["real"].clone().requires_grad_(True), t["fake"], SC, 0.8, 100, t["h_fake"], t["m_real"],
                                t["h_real"], t["m_fake"], ground_cost="l1").backward()


def test_l2_returns_the_bits_it_returns_without_the_keyword():
    G = _G()
    t = _loss_inputs("noise", 8, 43)
    a, ga = _gpu_loss(t)
    b, gb = _gpu_loss(t, ground_cost="l2")
    c, gc = _gpu_loss(t, ground_cost="l1")
    assert torch.equal(a, b) and all(torch.equal(ga[k], gb[k]) for k in WRT)
    assert float(c) != float(a)
    x, y = t["real"], t["fake"]
    assert torch.equal(G.cost_xy(x, y, SC), G.cost_xy(x, y, SC, ground_cost="l2"))
    assert torch.equal(G.modified_cost(x, y, t["h_fake"], t["m_real"], SC),
                       G.modified_cost(x, y, t["h_fake"], t["m_real"], SC, ground_cost="l2"))


def test_l1_loss_graph_replay_equals_eager():
    t = _loss_inputs("noise", 8, 45)
    for k in WRT:
        t[k].requires_grad_(True)
    G = _G()

    def step():
        loss = G.compute_sinkhorn_loss(t["real"], t["fake"], SC, 0.8, 100, t["h_fake"], t["m_real"], t["h_real"], t["m_fake"],
                                       ground_cost="l1")
        return [loss.detach().clone()] + [x.clone() for x in torch.autograd.grad(loss, [t[k] for k in WRT])]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for replay in range(2):
        if replay:
            with torch.no_grad():
                t["fake"].copy_(lo.videos("noise", 8, 46, DEV)[1])
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)


# ---- the public functions ----------------------------------------------------------------------------------------------------
def test_public_cost_functions_and_solvers_with_l1():
    G = _G()
    _lib()
    B1, B2, K = 5, 7, 40
    x, y = (v.view(-1, 8, 5) for v in lo.rows("ties", B1, B2, K, 51, DEV))
    hy, Mx, hx, My = _feats(B1, B2, 52)
    xd, yd = x.reshape(B1, -1).double(), y.reshape(B2, -1).double()
    l1 = lo.l1_block(xd, yd, SC)
    c1, c2 = _causal(hy, Mx)[0], _causal(hx, My)[0]
    tol = lambda ref: 2e-6 * float(ref.abs().max())     # (19 2^-24 of the L1 part, the causal terms' float32 dot products)
    for got, ref in ((G.cost_xy(x, y, SC, ground_cost="l1"), l1), (G.modified_cost(x, y, hy, Mx, SC, ground_cost="l1"), l1 + c1),
                     (G.bi_causal_modified_cost(x, y, hy, Mx, hx, My, SC, ground_cost="l1"), l1 + c1 + c2)):
        assert float((got.double() - ref).abs().max()) <= tol(ref)
    same = G.cost_xy(x, x, SC, ground_cost="l1")
    assert bool((same.diagonal() == 0).all()) and torch.equal(same, same.t())
    # the solvers, with gradients w.r.t. both operands (and the features)
    xs, ys = x.reshape(B1, -1), y.reshape(B2, -1)[:B1]                   # the solvers take square problems
    ref_b = ot.sinkhorn_from_cost(lo.l1_block(xs.double(), ys.double(), SC).cpu(), 1.0, 10, 10, stop_on_index=True)[0]
    got_b = G.benchmark_sinkhorn(xs.view(B1, 8, 5), ys.view(B1, 8, 5), SC, ground_cost="l1")
    assert abs(float(got_b) - float(ref_b)) <= 1e-4 * abs(float(ref_b))
    hs, Ms = hy, Mx[:B1]
    leaves = [v.detach().clone().requires_grad_(True) for v in (xs, ys, hs, Ms)]
    w = G.compute_sinkhorn(leaves[0].view(B1, 8, 5), leaves[1].view(B1, 8, 5), leaves[2], leaves[3], SC, ground_cost="l1")
    got = torch.autograd.grad(w, leaves)
    dl = [v.detach().double().cpu().requires_grad_(True) for v in (xs, ys, hs, Ms)]
    wr = ot.sinkhorn_from_cost(lo.l1_block(dl[0], dl[1], SC) + ot.causal_term(dl[2], dl[3], SC), 1.0, 100)[0]
    ref = torch.autograd.grad(wr, dl)
    assert abs(float(w) - float(wr)) <= 1e-4 * abs(float(wr))
    for name, a, b in zip(("x", "y", "h", "M"), got, ref):
        assert float((a.double().cpu() - b).abs().max()) <= 1e-4 * float(b.abs().max()), name
    # x is y: one tensor, its whole gradient once
    xv = xs.detach().clone().requires_grad_(True)
    gs = lo.upstream((B1, B1), 53, DEV)
    (G.cost_xy(xv, xv, SC, ground_cost="l1") * gs).sum().backward()
    rs = lo.adjoint_same(gs.double(), xs.double(), SC)
    assert float((xv.grad.double() - rs).abs().max()) <= 1e-5 * float(rs.abs().max())


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def test_trainer_with_the_l1_ground_cost(monkeypatch):
    from kccotgan_amd import gan, gan_utils
    from kccotgan_amd.kernel_train import KCCOTTrainer
    monkeypatch.setattr(gan, "_NATIVE", {"convlstm", "deconv", "dconv"})
    B, H, W, C, T, iT = 2, 64, 64, 1, 6, 2
    first = {}
    for gc in ("l1", "l2"):
        tr = KCCOTTrainer(B, total_time_steps=T, int_time_steps=iT, x_height=H, x_width=W, channels=C, kernel="1d", warmup=10,
                          device=DEV, ground_cost=gc)
        before = [p.detach().clone() for p in tr.g_params]
        g = torch.Generator().manual_seed(7)
        batches = [torch.rand((B, H, T, W, C), generator=g) for _ in range(2)]
        gan_utils.last_info.clear()
        out = tr.fit(iter(batches), log=None)
        assert out["iterations"] == 2 and not out["exploded"]
        finite = lambda v: v == v and abs(v) != float("inf")
        assert all(map(finite, out["history"]["Sinkhorn Loss"])) and all(map(finite, out["history"]["pM"]))
        assert any(not torch.equal(a, p.detach()) for a, p in zip(before, tr.g_params)), "the generator did not move"
        assert "compute_sinkhorn_loss_costs" in gan_utils.last_info
        first[gc] = out["history"]["Sinkhorn Loss"][0]
    assert first["l1"] != first["l2"]
