"""The weighted-marginal Sinkhorn solver and loss on the device (include/kccot_weighted.h, gan_utils.compute_weighted_sinkhorn /
compute_weighted_sinkhorn_loss) held to the float64 yardstick of tests/test_weighted_sinkhorn_cpu.py.

Tolerance (measured, not invented): in the same test the EXISTING uniform entry points
(kccot_sinkhorn_fwd_f32 / _bwd_f32, compute_sinkhorn_loss) are measured against float64 on the same inputs; that relative error
comes from the parent's kernels and is the yardstick.  A weighted result must satisfy
    |weighted - ref| <= 4 max(yardstick, 2^-24) max|ref|
per quantity (cost, dC; loss, dfake, each feature gradient).  Every test prints its figures before it asserts (-s).

Every buffer handed to the C ABI lies between NaN-filled guard zones that are verified after each call, workspaces are exactly as
long as the query says, and the rejected calls of the EINVAL matrix must leave every output untouched.
"""
import functools

import numpy as np
import pytest
import torch

import test_weighted_sinkhorn_cpu as W
from test_weighted_sinkhorn_cpu import F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
PAD = 64
FLOOR = 2.0 ** -24
FACTOR = 4.0
GCOST = (1.0, -0.5, 2.0)            # upstream gradient of the three costs of a launch
STOP_COUNT = 0


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


class Buf:
    """A device tensor of `shape` inside a NaN-filled allocation (int32: a NaN bit pattern), PAD elements of guard zone on either
    side."""

    def __init__(self, shape, src=None, dtype=F32):
        n = int(np.prod(shape))
        self.n, self.dtype = n, dtype
        self.raw = torch.full((n + 2 * PAD,), float("nan"), device=DEV, dtype=F32)
        self.t = self.raw[PAD:PAD + n].view(dtype).view(tuple(shape))
        if src is not None:
            self.t.copy_(src)

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.raw[:PAD]).all()) and bool(torch.isnan(self.raw[PAD + self.n:]).all())

    def untouched(self):
        return bool(torch.isnan(self.raw).all())


def workspace(nbytes):
    assert nbytes % 4 == 0
    return Buf((max(nbytes // 4, 1),)), nbytes


def call(L, name, *args, want=0):
    rc = getattr(L.lib, name)(*args)
    torch.cuda.synchronize()
    assert rc == want, "%s returned %d (wanted %d): %s" % (name, rc, want, L.lib.kccot_last_error().decode())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class OffsetBuf(Buf):
    """Buf whose tensor starts `off` floats past the allocation's aligned start: off = 1 puts it 4 bytes off a 16-byte boundary.
    The skipped floats stay NaN and count as guard zone."""

    def __init__(self, shape, src, off):
        n = int(np.prod(shape))
        super().__init__((n + off,))
        assert self.t.data_ptr() % 16 == 0
        self.off = off
        self.t = self.t[off:].view(tuple(shape))
        self.t.copy_(src)

    def guards_intact(self):
        return super().guards_intact() and bool(torch.isnan(self.raw[PAD:PAD + self.off]).all())


def solve(L, C, a, b, eps, Lit, gcost=GCOST, bwd=True, c_off=0):
    """cost [nprob], nits [2 nprob], dC [nprob,n,n] through the C ABI; a = b = None: the existing uniform entry points.
    c_off: C starts that many floats past a 16-byte boundary (every other buffer stays aligned)."""
    nprob, n, _ = C.shape
    Lh = max(Lit, 1)
    bufs = {"C": OffsetBuf(C.shape, C, c_off), "u": Buf((nprob, Lh, n)), "v": Buf((nprob, Lh, n)), "cost": Buf((nprob,)),
            "nits": Buf((2 * nprob,), dtype=torch.int32), "dC": Buf(C.shape), "g": Buf((nprob,), torch.tensor(gcost[:nprob]))}
    ws, wsb = workspace(L.lib.kccot_sinkhorn_workspace_bytes(nprob, n))
    bufs["ws"] = ws
    wp = ws.ptr() if wsb else None
    if a is None:
        call(L, "kccot_sinkhorn_fwd_f32", bufs["C"].ptr(), nprob, n, eps, Lit, W.LMIN, W.THRESH, STOP_COUNT, bufs["u"].ptr(),
             bufs["v"].ptr(), bufs["cost"].ptr(), bufs["nits"].ptr(), None, wp, wsb, None)
        if bwd:
            call(L, "kccot_sinkhorn_bwd_f32", bufs["C"].ptr(), bufs["u"].ptr(), bufs["v"].ptr(), bufs["nits"].ptr(), nprob, n,
                 eps, Lh, bufs["g"].ptr(), bufs["dC"].ptr(), wp, wsb, None)
    else:
        bufs["a"], bufs["b"] = Buf(a.shape, a), Buf(b.shape, b)
        call(L, "kccot_sinkhorn_weighted_fwd_f32", bufs["C"].ptr(), bufs["a"].ptr(), bufs["b"].ptr(), nprob, n, eps, Lit, W.LMIN,
             W.THRESH, STOP_COUNT, bufs["u"].ptr(), bufs["v"].ptr(), bufs["cost"].ptr(), bufs["nits"].ptr(), None, wp, wsb, None)
        if bwd:
            call(L, "kccot_sinkhorn_weighted_bwd_f32", bufs["C"].ptr(), bufs["a"].ptr(), bufs["b"].ptr(), bufs["u"].ptr(),
                 bufs["v"].ptr(), bufs["nits"].ptr(), nprob, n, eps, Lh, bufs["g"].ptr(), bufs["dC"].ptr(), wp, wsb, None)
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d)" % (k, n)
    return bufs["cost"].t.clone(), bufs["nits"].t.clone(), bufs["dC"].t.clone()


# ---------------------------------------------------------------- inputs and float64 references, computed once
@functools.lru_cache(maxsize=None)
def problems(n):
    """C [3,n,n] float32, a, b [3,n] float64 (normalised; their float32 roundings are what the device reads)."""
    C = torch.stack([W.small_cost(n, 100 * n + p) for p in range(3)])
    a = torch.stack([W.random_weights(n, 1000 + 10 * n + p) for p in range(3)]).float()
    b = torch.stack([W.random_weights(n, 2000 + 10 * n + p) for p in range(3)]).float()
    return C, a, b


@functools.lru_cache(maxsize=None)
def reference(n, eps, Lit, uniform):
    """float64 (cost [3], nits [3], dC [3,n,n]) for sum_p GCOST[p] cost[p] on the float32 inputs the device reads."""
    C, a, b = problems(n)
    C64 = C.double().requires_grad_(True)
    costs, nits = [], []
    for p in range(3):
        wa = torch.full((n,), 1.0 / n, dtype=F64) if uniform else a[p].double()
        wb = torch.full((n,), 1.0 / n, dtype=F64) if uniform else b[p].double()
        c, k, _ = W.weighted_sinkhorn(C64[p], wa, wb, eps, Lit)
        costs.append(c)
        nits.append(k)
    (dC,) = torch.autograd.grad(sum(g * c for g, c in zip(GCOST, costs)), C64)
    return torch.stack(costs).detach(), nits, dC


def rel_err(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()) / float(ref.abs().max())


def within(tag, got, ref, yard):
    """Assert |got - ref| <= FACTOR max(yard, FLOOR) max|ref|; returns the error as a multiple of max(yard, FLOOR)."""
    e = rel_err(got, ref)
    ratio = e / max(yard, FLOOR)
    print("%-40s err %.3e  yardstick %.3e  ratio %.2f (cap %g)" % (tag, e, yard, ratio, FACTOR))
    assert bool(torch.isfinite(got).all()), tag
    assert ratio <= FACTOR, "%s: %.3e > %g x max(%.3e, 2^-24)" % (tag, e, FACTOR, yard)
    return ratio


SIZES = (5, 64, 67, 128, 130)
EPS_L = [(0.8, 7), (0.8, 100), (1.0, 7), (1.0, 100)]


# ================================================================ 1. fp64 parity through the C ABI
@pytest.mark.parametrize("eps,Lit", EPS_L)
@pytest.mark.parametrize("n", SIZES)
def test_solver_against_fp64(L, n, eps, Lit):
    C, a, b = problems(n)
    ref_u, ref_w = reference(n, eps, Lit, True), reference(n, eps, Lit, False)
    cost_u, nits_u, dC_u = solve(L, C, None, None, eps, Lit)
    yard_c, yard_d = rel_err(cost_u, ref_u[0]), rel_err(dC_u, ref_u[2])
    cost_w, nits_w, dC_w = solve(L, C, a, b, eps, Lit)
    assert nits_w[:3].tolist() == ref_w[1] == [Lit] * 3 and nits_u[:3].tolist() == ref_u[1]
    r1 = within("n=%d eps=%g L=%d cost" % (n, eps, Lit), cost_w, ref_w[0], yard_c)
    r2 = within("n=%d eps=%g L=%d dC" % (n, eps, Lit), dC_w, ref_w[2], yard_d)
    print("WORST n=%d: %.2f" % (n, max(r1, r2)))


# ================================================================ 2. uniform weights give the existing answer
@pytest.mark.parametrize("n", SIZES)
def test_uniform_weights_agree_with_the_existing_entry_points(L, n):
    eps, Lit = 1.0, 100
    C, _, _ = problems(n)
    ref_u = reference(n, eps, Lit, True)
    uni = torch.full((3, n), 1.0 / n, dtype=F32)
    cost_u, nits_u, dC_u = solve(L, C, None, None, eps, Lit)
    cost_w, nits_w, dC_w = solve(L, C, uni, uni, eps, Lit)
    assert nits_w[:3].tolist() == nits_u[:3].tolist()
    within("n=%d uniform cost vs existing" % n, cost_w, cost_u.double().cpu(), rel_err(cost_u, ref_u[0]))
    within("n=%d uniform dC vs existing" % n, dC_w, dC_u.double().cpu(), rel_err(dC_u, ref_u[2]))


# ================================================================ 3. / 4. the loss
LOSS_SHAPES = [(6, 4, 8, 8, 1, 3), (64, 5, 8, 8, 1, 4)]          # (B, T, H, W, C, J)
LOSS_EPS, LOSS_L = 0.8, 100
FEATS = ("h_fake", "m_real", "h_real", "m_fake")


@functools.lru_cache(maxsize=None)
def loss_inputs(shape):
    B, T, H, Wd, Cc, J = shape
    rng = np.random.default_rng(7 + B)
    t = {"real": rng.random((B, H, T, Wd, Cc), dtype=np.float32), "fake": rng.random((B, H, T, Wd, Cc), dtype=np.float32)}
    t.update({k: rng.random((B, T, J), dtype=np.float32) for k in FEATS})
    t = {k: torch.from_numpy(v) for k, v in t.items()}
    t["w_real"], t["w_fake"] = W.random_weights(B, 31 + B).float(), W.random_weights(B, 47 + B).float()
    return t


def loss_reference_with(shape, a, b, Lit=LOSS_L):
    """float64 (loss, dfake, dh_fake, dm_real, dh_real, dm_fake) with marginals a, b (float64 [B])."""
    t = loss_inputs(shape)
    d = {k: t[k].double() for k in ("real", "fake") + FEATS}
    leaves = [d[k].requires_grad_(True) for k in ("fake",) + FEATS]
    loss, _, nits = W.weighted_loss(d["real"], d["fake"], W.cases.SC, LOSS_EPS, Lit, d["h_fake"], d["m_real"], d["h_real"],
                                    d["m_fake"], a, b)
    assert nits == (Lit,) * 3
    return (loss.detach(),) + torch.autograd.grad(loss, leaves)


@functools.lru_cache(maxsize=None)
def loss_reference(shape, uniform):
    t = loss_inputs(shape)
    B = shape[0]
    if uniform:
        return loss_reference_with(shape, torch.full((B,), 1.0 / B, dtype=F64), torch.full((B,), 1.0 / B, dtype=F64))
    return loss_reference_with(shape, t["w_real"].double(), t["w_fake"].double())


def run_loss(shape, w_real=None, w_fake=None, normalize=False, Lit=LOSS_L, weight_grads=False):
    """(loss, dfake, four feature gradients) of compute_weighted_sinkhorn_loss, or of compute_sinkhorn_loss without weights.
    weight_grads: the weights require a gradient, and (dw_real, dw_fake) follow the six."""
    from kccotgan_amd import gan_utils as g
    t = loss_inputs(shape)
    real = t["real"].to(DEV)
    leaves = [t[k].to(DEV).requires_grad_(True) for k in ("fake",) + FEATS]
    fake, hf, mr, hr, mf = leaves
    if w_real is None:
        loss = g.compute_sinkhorn_loss(real, fake, W.cases.SC, LOSS_EPS, Lit, hf, mr, hr, mf, honor_eps_l=True)
    else:
        wr, wf = w_real.to(DEV).requires_grad_(weight_grads), w_fake.to(DEV).requires_grad_(weight_grads)
        loss = g.compute_weighted_sinkhorn_loss(real, fake, W.cases.SC, LOSS_EPS, Lit, hf, mr, hr, mf, wr, wf, normalize=normalize)
        if weight_grads:
            leaves = leaves + [wr, wf]
    grads = torch.autograd.grad(loss, leaves)
    torch.cuda.synchronize()
    return (loss.detach(),) + grads


NAMES = ("loss", "dfake", "dh_fake", "dm_real", "dh_real", "dm_fake")


@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_loss_against_fp64(shape):
    t = loss_inputs(shape)
    ref_u, ref_w = loss_reference(shape, True), loss_reference(shape, False)
    got_u = run_loss(shape)
    got_w = run_loss(shape, t["w_real"], t["w_fake"])
    worst = 0.0
    for k, gu, ru, gw, rw in zip(NAMES, got_u, ref_u, got_w, ref_w):
        worst = max(worst, within("%s %s" % (shape, k), gw, rw.reshape(gw.shape), rel_err(gu, ru.reshape(gu.shape))))
    print("WORST loss %s: %.2f" % (shape, worst))


@pytest.mark.parametrize("shape", LOSS_SHAPES)
def test_normalize_divides_by_the_sum_on_the_device(shape):
    t = loss_inputs(shape)
    a73, b73 = t["w_real"] * 7.3, t["w_fake"] * 7.3
    got = run_loss(shape, a73, b73, normalize=True)
    a_pre, b_pre = a73.to(DEV) / a73.to(DEV).sum(), b73.to(DEV) / b73.to(DEV).sum()
    pre = run_loss(shape, a_pre, b_pre, normalize=False)
    assert all(same_bits(x, y) for x, y in zip(got, pre))
    assert abs(float(a_pre.sum()) - 1.0) < 1e-6


def test_weights_change_the_answer():
    """Permuting w_fake moves the loss by more than 100 x the tolerance: on the float64 reference first, then on the device."""
    shape = LOSS_SHAPES[1]
    t = loss_inputs(shape)
    B = shape[0]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5))
    ref = loss_reference(shape, False)[0]
    ref_p = loss_reference_with(shape, t["w_real"].double(), t["w_fake"][perm].double())[0]
    yard = rel_err(run_loss(shape)[0], loss_reference(shape, True)[0])
    tol = FACTOR * max(yard, FLOOR) * abs(float(ref))
    print("reference loss %.6f, permuted %.6f, gap %.3e, tolerance %.3e" % (float(ref), float(ref_p), abs(float(ref - ref_p)), tol))
    assert abs(float(ref) - float(ref_p)) > 100 * tol
    got = run_loss(shape, t["w_real"], t["w_fake"])[0]
    got_p = run_loss(shape, t["w_real"], t["w_fake"][perm])[0]
    assert abs(float(got) - float(got_p)) > 100 * tol
    within("permuted loss", got_p, ref_p.reshape(()), yard)


# ================================================================ 5. bad weights surface
@pytest.mark.parametrize("bad", [0.0, -0.25, float("nan")])
@pytest.mark.parametrize("n", [64, 130])
def test_a_bad_weight_poisons_its_problem_only(L, n, bad):
    C, a, b = problems(n)
    good = solve(L, C, a, b, 1.0, 7)
    for side in (0, 1):
        a2, b2 = a.clone(), b.clone()
        (a2, b2)[side][1, n // 3] = bad
        cost, nits, dC = solve(L, C, a2, b2, 1.0, 7)
        assert not bool(torch.isfinite(cost[1])) and int(nits[1]) < 0, (cost, nits)
        assert bool(torch.isnan(dC[1]).all())
        for p in (0, 2):
            assert same_bits(cost[p], good[0][p]) and int(nits[p]) == 7 and same_bits(dC[p], good[2][p])


@pytest.mark.parametrize("bad", [0.0, -0.25, float("nan")])
def test_raise_if_solver_aborted_reports_a_bad_weight(L, bad):
    from kccotgan_amd import gan_utils as g
    shape = LOSS_SHAPES[0]
    t = loss_inputs(shape)
    w = t["w_fake"].clone()
    w[2] = bad
    got = run_loss(shape, t["w_real"], w)
    assert not bool(torch.isfinite(got[0])) and not bool(torch.isfinite(got[1]).any())
    with pytest.raises(L.KccotError, match="weight"):
        g.raise_if_solver_aborted(("compute_weighted_sinkhorn_loss",))
    run_loss(shape, t["w_real"], t["w_fake"])
    g.raise_if_solver_aborted(("compute_weighted_sinkhorn_loss",))        # good weights: nothing to report


# ================================================================ 6. batch-position independence
@pytest.mark.parametrize("n", SIZES)
def test_cost_bits_do_not_depend_on_nprob(L, n):
    C, a, b = problems(n)
    full = solve(L, C, a, b, 1.0, 100)
    for p in range(3):
        one = solve(L, C[p:p + 1].contiguous(), a[p:p + 1].contiguous(), b[p:p + 1].contiguous(), 1.0, 100, gcost=GCOST[p:p + 1])
        assert same_bits(one[0][0], full[0][p]) and same_bits(one[2][0], full[2][p]), (n, p)


# ================================================================ 7. routing
def test_routing_register_streaming_and_never_multi_cu(L):
    from kccotgan_amd import gan_utils as g
    assert L.get_option("sinkhorn_coop") == 1 and L.get_option("sinkhorn_fused") == 1
    assert L.lib.kccot_sinkhorn_fused_eligible(64, LOSS_L) == 1       # the unweighted loss WOULD take the fused launch here
    for B, path in ((64, "register"), (130, "streaming")):
        rng = np.random.default_rng(B)
        real, fake = (torch.from_numpy(rng.random((B, 2, 3, 4, 1), dtype=np.float32)).to(DEV) for _ in range(2))
        feats = [torch.from_numpy(rng.random((B, 3, 2), dtype=np.float32)).to(DEV) for _ in range(4)]
        fake.requires_grad_(True)
        w = W.random_weights(B, B).float().to(DEV)
        loss = g.compute_weighted_sinkhorn_loss(real, fake, 1.0, 1.0, 20, *feats, w, w, normalize=False)
        (dfake,) = torch.autograd.grad(loss, fake)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dfake).all())
        assert g.last_info["compute_weighted_sinkhorn_loss_fused_sweep"] is False
        assert g.last_info["compute_weighted_sinkhorn_loss_path"] == path
        assert g.last_info["compute_weighted_sinkhorn_loss"].tolist() == [20, 20, 20]
        # the solve the wrapper reports is the solve that ran: the ABI's weighted entry point on the same matrices, which has
        # no multi-CU form, gives the same cost bits
        C3 = g.last_info["compute_weighted_sinkhorn_loss_C3"].cpu()
        w3a, w3b = torch.stack([w, w, w]).cpu(), torch.stack([w, w, w]).cpu()
        cost, _, _ = solve(L, C3, w3a, w3b, 1.0, 20, bwd=False)
        assert same_bits(cost, g.last_info["compute_weighted_sinkhorn_loss_costs"])
    x, y = torch.rand(130, 3, 4, device=DEV), torch.rand(130, 3, 4, device=DEV)
    h, M = torch.rand(130, 3, 2, device=DEV), torch.rand(130, 3, 2, device=DEV)
    w = W.random_weights(130, 1).float().to(DEV)
    c = g.compute_weighted_sinkhorn(x, y, h, M, 1.0, w, w, epsilon=1.0, L=10)
    assert bool(torch.isfinite(c)) and g.last_info["compute_weighted_sinkhorn_path"] == "streaming"


# ================================================================ the loss entry points through the C ABI, guarded
def loss_abi(L, shape, w_real, w_fake):
    t = loss_inputs(shape)
    B, T, H, Wd, Cc, J = shape
    K = T * H * Wd * Cc
    Lh = LOSS_L
    ins = {k: Buf(t[k].reshape(B, -1).shape if k in ("real", "fake") else t[k].shape, t[k].reshape(B, -1) if k in ("real", "fake")
                  else t[k]) for k in ("real", "fake") + FEATS}
    ins["w_real"], ins["w_fake"], ins["g"] = Buf((B,), w_real), Buf((B,), w_fake), Buf((1,), torch.ones(1))
    out = {"C3": Buf((3, B, B)), "u": Buf((3, Lh, B)), "v": Buf((3, Lh, B)), "cost3": Buf((3,)),
           "nits": Buf((6,), dtype=torch.int32), "loss": Buf((1,)), "ticket": Buf((1,), torch.zeros(1, dtype=torch.int32), torch.int32),
           "dfake": Buf((B, K)), "dh_fake": Buf((B, T, J)), "dh_real": Buf((B, T, J)), "dm_real": Buf((B, T, J)),
           "dm_fake": Buf((B, T, J))}
    ws, wsb = workspace(L.lib.kccot_weighted_sinkhorn_loss_workspace_bytes(B, K))
    out["ws"] = ws
    feats = [ins[k].ptr() for k in ("h_fake", "h_real", "m_real", "m_fake")]
    call(L, "kccot_weighted_sinkhorn_loss_fwd_f32", ins["real"].ptr(), ins["fake"].ptr(), B, K, W.cases.SC, *feats, T, J, LOSS_EPS,
         LOSS_L, W.LMIN, W.THRESH, 0, ins["w_real"].ptr(), ins["w_fake"].ptr(), out["C3"].ptr(), out["u"].ptr(), out["v"].ptr(),
         out["cost3"].ptr(), out["nits"].ptr(), out["loss"].ptr(), out["ticket"].ptr(), ws.ptr(), wsb, None)
    call(L, "kccot_weighted_sinkhorn_loss_bwd_f32", ins["g"].ptr(), ins["real"].ptr(), ins["fake"].ptr(), B, K, W.cases.SC, *feats, T,
         J, LOSS_EPS, Lh, ins["w_real"].ptr(), ins["w_fake"].ptr(), out["C3"].ptr(), out["u"].ptr(), out["v"].ptr(),
         out["nits"].ptr(), out["dfake"].ptr(), out["dh_fake"].ptr(), out["dh_real"].ptr(), out["dm_real"].ptr(),
         out["dm_fake"].ptr(), ws.ptr(), wsb, None)
    for k, bf in list(ins.items()) + list(out.items()):
        assert bf.guards_intact(), "guard zone of %s overwritten" % k
    assert int(out["ticket"].t) == 0
    return out


@pytest.mark.parametrize("shape", LOSS_SHAPES + [(130, 2, 4, 4, 1, 2)])
def test_loss_entry_points_through_the_abi_give_the_wrappers_bits(L, shape):
    t = loss_inputs(shape)
    out = loss_abi(L, shape, t["w_real"], t["w_fake"])
    got = run_loss(shape, t["w_real"], t["w_fake"])
    B = shape[0]
    pairs = (("loss", got[0]), ("dfake", got[1]), ("dh_fake", got[2]), ("dm_real", got[3]), ("dh_real", got[4]), ("dm_fake", got[5]))
    for k, g in pairs:
        assert bool(torch.isfinite(out[k].t).all()), k
        assert same_bits(out[k].t.reshape(-1), g.reshape(-1)), k
    assert out["nits"].t[:3].tolist() == [LOSS_L] * 3


# ================================================================ 8. the EINVAL matrix, in-process, every output guarded
def test_rejected_calls_leave_every_output_untouched(L):
    EINVAL, EWORKSPACE = L.EINVAL, L.EWORKSPACE
    for n in (64, 130):
        C, a, b = problems(n)
        nprob, Lit = 3, 7
        Cb, ab, bb = Buf(C.shape, C), Buf(a.shape, a), Buf(b.shape, b)
        outs = {k: Buf(s) for k, s in (("u", (nprob, Lit, n)), ("v", (nprob, Lit, n)), ("cost", (nprob,)), ("nits", (2 * nprob,)),
                                       ("dC", C.shape))}
        g = Buf((nprob,), torch.tensor(GCOST))
        need = L.lib.kccot_sinkhorn_workspace_bytes(nprob, n)
        ws, wsb = workspace(need)
        wp = ws.ptr() if need else None

        def fwd(a_=ab.ptr(), b_=bb.ptr(), n_=n, wsb_=wsb, want=EINVAL):
            call(L, "kccot_sinkhorn_weighted_fwd_f32", Cb.ptr(), a_, b_, nprob, n_, 1.0, Lit, W.LMIN, W.THRESH, STOP_COUNT,
                 outs["u"].ptr(), outs["v"].ptr(), outs["cost"].ptr(), outs["nits"].ptr(), None, wp, wsb_, None, want=want)

        def bwd(a_=ab.ptr(), b_=bb.ptr(), n_=n, wsb_=wsb, want=EINVAL):
            call(L, "kccot_sinkhorn_weighted_bwd_f32", Cb.ptr(), a_, b_, outs["u"].ptr(), outs["v"].ptr(), outs["nits"].ptr(), nprob,
                 n_, 1.0, Lit, g.ptr(), outs["dC"].ptr(), wp, wsb_, None, want=want)

        for f in (fwd, bwd):
            f(a_=None)
            f(b_=None)
            f(n_=0)
            f(n_=-3)
            if need:                      # one byte short (n <= 128 needs no workspace at all)
                f(wsb_=need - 1, want=EWORKSPACE)
        assert all(o.untouched() for o in outs.values()) and ws.untouched()
    # the loss entry points
    shape = LOSS_SHAPES[0]
    t = loss_inputs(shape)
    B, T, H, Wd, Cc, J = shape
    K = T * H * Wd * Cc
    ins = {k: Buf((B, K) if k in ("real", "fake") else t[k].shape, t[k].reshape(B, -1) if k in ("real", "fake") else t[k])
           for k in ("real", "fake") + FEATS}
    wr, wf, g1 = Buf((B,), t["w_real"]), Buf((B,), t["w_fake"]), Buf((1,), torch.ones(1))
    outs = {k: Buf(s) for k, s in (("C3", (3, B, B)), ("u", (3, 7, B)), ("v", (3, 7, B)), ("cost3", (3,)), ("nits", (6,)),
                                   ("loss", (1,)), ("dfake", (B, K)), ("dh_fake", (B, T, J)), ("dh_real", (B, T, J)),
                                   ("dm_real", (B, T, J)), ("dm_fake", (B, T, J)))}
    ticket = Buf((1,), torch.zeros(1, dtype=torch.int32), torch.int32)
    need = L.lib.kccot_weighted_sinkhorn_loss_workspace_bytes(B, K)
    ws, wsb = workspace(need)
    feats = [ins[k].ptr() for k in ("h_fake", "h_real", "m_real", "m_fake")]

    def lfwd(wr_=wr.ptr(), wf_=wf.ptr(), B_=B, wsb_=wsb, want=EINVAL):
        call(L, "kccot_weighted_sinkhorn_loss_fwd_f32", ins["real"].ptr(), ins["fake"].ptr(), B_, K, 1.0, *feats, T, J, 1.0, 7, W.LMIN,
             W.THRESH, 0, wr_, wf_, outs["C3"].ptr(), outs["u"].ptr(), outs["v"].ptr(), outs["cost3"].ptr(), outs["nits"].ptr(),
             outs["loss"].ptr(), ticket.ptr(), ws.ptr(), wsb_, None, want=want)

    def lbwd(wr_=wr.ptr(), wf_=wf.ptr(), B_=B, wsb_=wsb, want=EINVAL):
        call(L, "kccot_weighted_sinkhorn_loss_bwd_f32", g1.ptr(), ins["real"].ptr(), ins["fake"].ptr(), B_, K, 1.0, *feats, T, J, 1.0, 7,
             wr_, wf_, outs["C3"].ptr(), outs["u"].ptr(), outs["v"].ptr(), outs["nits"].ptr(), outs["dfake"].ptr(),
             outs["dh_fake"].ptr(), outs["dh_real"].ptr(), outs["dm_real"].ptr(), outs["dm_fake"].ptr(), ws.ptr(), wsb_, None,
             want=want)

    for f in (lfwd, lbwd):
        f(wr_=None)
        f(wf_=None)
        f(B_=0)
        f(wsb_=need - 1, want=EWORKSPACE)
    assert all(o.untouched() for o in outs.values()) and ws.untouched() and int(ticket.t) == 0
