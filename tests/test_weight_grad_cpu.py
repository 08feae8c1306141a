"""CPU tier of the WEIGHT gradients of the weighted Sinkhorn solver and of the kernel-conditional loss
(include/kccot_weight_grad.h, gan_utils.compute_weighted_sinkhorn[_loss] w.r.t. their weights,
gan_utils.compute_kernel_conditional_sinkhorn_loss): the yardsticks the GPU tier (tests/test_gpu_weight_grad.py) is held to,
proved here against float64 autograd, plus the header, the ctypes table, the argument validation and the Python surface.

The yardstick is the reverse sweep in plain torch, parametrised by dtype and sharing no code with the library: with gu_t the
adjoint of u_t after the row pass of iteration t and gv_t the adjoint of v_t when that pass starts (gv_nits: the final-cost term;
the adjoint of v_0 = 0 is a constant's and is not added),

    dW/da_i = (eps / a_i) sum_{t=1..nits} gu_t[i],          dW/db_j = (eps / b_j) sum_{t=1..nits} gv_t[j].

Its float32 run against its float64 run on the same inputs is the error yardstick of the device's da and db.
"""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import test_conditional_sinkhorn_cpu as CC
import test_weighted_sinkhorn_cpu as W
from test_weighted_sinkhorn_cpu import F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_W = 2.0 ** -100


# ================================================================ the yardsticks
def sweep(C, a, b, eps, L, g=1.0, dtype=F64, Lmin=W.LMIN, add_v0=False):
    """(cost, nits, dC, da, db) of g W(C; a, b): the weighted loop of kccot_weighted.h run forward with its history kept, then
    the reverse sweep with the two sums.  Every operation in `dtype`.  add_v0: (wrongly) add the adjoint of v_0 too."""
    C, a, b = C.to(dtype), a.to(dtype), b.to(dtype)
    la, lb = torch.log(a), torch.log(b)
    U, V = [torch.zeros_like(a)], [torch.zeros_like(b)]
    nits = 0
    for _ in range(int(L)):
        u = eps * (la - torch.logsumexp((-C + U[-1][:, None] + V[-1][None, :]) / eps, dim=1)) + U[-1]
        v = eps * (lb - torch.logsumexp((-C + u[:, None] + V[-1][None, :]) / eps, dim=0)) + V[-1]
        err = float((u - U[-1]).abs().sum())
        U.append(u)
        V.append(v)
        nits += 1
        if W.THRESH > err and nits >= Lmin:
            break
    pi = torch.exp((-C + U[nits][:, None] + V[nits][None, :]) / eps)
    cost = (pi * C).sum()
    dC = g * pi * (1.0 - C / eps)
    gu = g * (pi * C).sum(1) / eps
    gv = g * (pi * C).sum(0) / eps
    sa = torch.zeros_like(a)
    sb = gv.clone() if nits > 0 else torch.zeros_like(b)
    for t in range(nits, 0, -1):
        Qt = torch.exp((-C + U[t][:, None] + (V[t] - eps * lb)[None, :]) / eps)          # column sums 1: dv_t/du_t = -Qt
        w = Qt * gv[None, :]
        dC = dC + w
        gu = (gu if t == nits else torch.zeros_like(gu)) - w.sum(1)
        sa = sa + gu
        Pt = torch.exp((-C + (U[t] - eps * la)[:, None] + V[t - 1][None, :]) / eps)      # row sums 1: du_t/dv_{t-1} = -Pt
        w = Pt * gu[:, None]
        dC = dC + w
        gv = -w.sum(0)
        if t > 1 or add_v0:                         # t == 1: the adjoint of v_0 = 0, a constant
            sb = sb + gv
    return cost, nits, dC, eps * sa / a, eps * sb / b


def weights_adjoint(D, w, dw, bw, dtype=F64):
    """(dD [Q,n], dbw [Q]) of w = max(softmax(-D / (2 bw^2)), 2^-100) from the STORED weights w and their gradient dw; the
    floor has zero slope.  Every operation in `dtype`."""
    D, w, dw = D.to(dtype), w.to(dtype), dw.to(dtype)
    live = w > FLOOR_W
    zero = torch.zeros_like(w)
    m = torch.where(live, w * dw, zero).sum(1, keepdim=True)
    dl = torch.where(live, w * (dw - m), zero)
    return -dl / (2.0 * bw * bw), (dl * D).sum(1) / (bw ** 3)


# ================================================================ 1. the sweep's formula against float64 autograd
@pytest.mark.parametrize("eps", [0.8, 1.0])
@pytest.mark.parametrize("L", [1, 12])            # L = 1: the case the "adjoint of v_0 is not added" rule decides
@pytest.mark.parametrize("n", [6, 17])
def test_sweep_matches_autograd_of_the_yardstick(n, L, eps):
    C = W.small_cost(n, 40 + n).double()
    a, b = W.random_weights(n, 3 + n), W.random_weights(n, 4 + n)
    for same in (False, True):
        Cl, al, bl = C.clone().requires_grad_(True), a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        cost, nits, _ = W.weighted_sinkhorn(Cl, al, al if same else bl, eps, L)
        if same:
            rC, ra = torch.autograd.grad(cost, (Cl, al))
        else:
            rC, ra, rb = torch.autograd.grad(cost, (Cl, al, bl))
        got_cost, got_nits, dC, da, db = sweep(C, a, a if same else b, eps, L)
        assert got_nits == nits == L
        assert abs(float(got_cost) - float(cost)) <= 1e-12 * abs(float(cost))
        pairs = [("dC", dC, rC), ("da+db", da + db, ra)] if same else [("dC", dC, rC), ("da", da, ra), ("db", db, rb)]
        for name, got, ref in pairs:
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            print("n=%d L=%d eps=%g same=%s %s: %.2e" % (n, L, eps, same, name, err))
            assert err <= 1e-10, (name, err)


def test_dropping_the_v0_rule_would_be_wrong_at_one_iteration():
    """At L = 1 the column pass writes the adjoint of v_0; adding it changes db by O(1): the rule is not a rounding matter."""
    n, eps = 6, 1.0
    C, a, b = W.small_cost(n, 46).double(), W.random_weights(n, 9), W.random_weights(n, 10)
    bl = b.clone().requires_grad_(True)
    (rb,) = torch.autograd.grad(W.weighted_sinkhorn(C, a, bl, eps, 1)[0], bl)
    _, _, _, _, db = sweep(C, a, b, eps, 1)
    assert float((db - rb).abs().max()) <= 1e-12 * float(rb.abs().max())
    wrong = sweep(C, a, b, eps, 1, add_v0=True)[4]
    assert float((wrong - rb).abs().max()) > 1e-2 * float(rb.abs().max())


def test_no_iteration_means_no_weight_gradient():
    n = 6
    C, a, b = W.small_cost(n, 47).double(), W.random_weights(n, 11), W.random_weights(n, 12)
    _, nits, _, da, db = sweep(C, a, b, 1.0, 0)
    assert nits == 0 and float(da.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


def test_float32_run_of_the_sweep_is_a_usable_yardstick():
    """float32 against float64 on the same inputs: small and non-zero (it is what the device's da / db are held to)."""
    n, eps, L = 17, 0.8, 12
    C, a, b = W.small_cost(n, 48), W.random_weights(n, 13).float(), W.random_weights(n, 14).float()
    r = sweep(C, a, b, eps, L)
    s = sweep(C, a, b, eps, L, dtype=torch.float32)
    for k in (2, 3, 4):
        err = float((s[k].double() - r[k]).abs().max()) / float(r[k].abs().max())
        assert 0.0 < err < 1e-4, (k, err)


# ================================================================ 2. the adjoint of the weight estimator
@pytest.mark.parametrize("bw,floored", [(0.9, False), (0.25, True)])
def test_weights_adjoint_matches_autograd(bw, floored):
    g = torch.Generator().manual_seed(17)
    c = 3.0 * torch.rand(9, 5, generator=g, dtype=F64)
    D = (torch.cdist(c[:3], c) ** 2).detach()
    dw = torch.randn(3, 9, generator=g, dtype=F64)
    Dl = D.clone().requires_grad_(True)
    bwl = torch.tensor(bw, dtype=F64, requires_grad=True)
    w = torch.clamp_min(torch.softmax(-Dl / (2.0 * bwl * bwl), dim=1), FLOOR_W)
    assert bool((w.detach() == CC.conditional_weights(D, bw)).all())
    n_floor = int((w.detach() == FLOOR_W).sum())
    assert (n_floor > 0) == floored, n_floor
    rD, rbw = torch.autograd.grad((w * dw).sum(), (Dl, bwl))
    dD, dbw = weights_adjoint(D, w.detach(), dw, bw)
    assert float((dD - rD).abs().max()) <= 1e-12 * max(float(rD.abs().max()), 1e-300)
    assert abs(float(dbw.sum()) - float(rbw)) <= 1e-12 * max(abs(float(rbw)), 1e-300)
    assert bool((dD[w.detach() == FLOOR_W] == 0).all())


# ================================================================ 3. header, ctypes table
def _decls():
    text = open(os.path.join(ROOT, "include", "kccot_weight_grad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_is_strict_c99_and_matches_the_ctypes_table(tmp_path):
    from kccotgan_amd import _lib
    decls = _decls()
    assert sorted(decls) == sorted(_lib.WEIGHT_GRAD_SIGNATURES), "ctypes table and header disagree"
    others = (set(_lib.SIGNATURES) | set(_lib.MODEL_SIGNATURES) | set(_lib.WEIGHTED_SIGNATURES) | set(_lib.CONDITIONAL_SIGNATURES) |
              set(_lib.SMOOTH3C_SIGNATURES))
    assert not set(_lib.WEIGHT_GRAD_SIGNATURES) & others
    for name in ("kccot_sinkhorn_weighted_bwd_dw_f32", "kccot_weighted_sinkhorn_loss_bwd_dw_f32",
                 "kccot_sinkhorn_conditional_dw_workspace_bytes", "kccot_sinkhorn_conditional_bwd_dw_f32",
                 "kccot_conditional_sinkhorn_loss_bwd_dw_f32", "kccot_conditional_weights_bwd_f32"):
        assert name in decls, name
    ctype = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "unsigned": ctypes.c_uint,
             "size_t": ctypes.c_size_t}
    for name, args in decls.items():
        assert hasattr(_lib.lib, name), "libkccot.so does not export %s" % name
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        assert _lib.WEIGHT_GRAD_SIGNATURES[name][1] == want, name
        assert getattr(_lib.lib, name).argtypes == want
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_weight_grad.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(probe), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ================================================================ 4. argument validation, before any launch
def test_argument_validation_happens_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)      # never dereferenced: every call below is rejected on its arguments
    EINVAL, EWORKSPACE, EUNSUPPORTED = _lib.EINVAL, _lib.EWORKSPACE, _lib.EUNSUPPORTED
    need130 = lib.kccot_sinkhorn_workspace_bytes(1, 130)

    def sbwd(C=one, a=one, b=one, uh=one, nits=one, nprob=1, n=8, eps=1.0, L=10, g=one, dC=one, da=one, db=one, ws=None, wsb=0):
        return lib.kccot_sinkhorn_weighted_bwd_dw_f32(C, a, b, uh, one, nits, nprob, n, eps, L, g, dC, da, db, ws, wsb, None)

    for kw in ({"C": None}, {"a": None}, {"b": None}, {"uh": None}, {"nits": None}, {"g": None}, {"dC": None}, {"da": None},
               {"db": None}, {"nprob": 0}, {"n": 0}, {"eps": 0.0}, {"eps": -1.0}, {"L": -1}):
        assert sbwd(**kw) == EINVAL, kw
    assert sbwd(n=130, ws=one, wsb=need130 - 1) == EWORKSPACE and sbwd(n=1025, ws=one, wsb=1 << 40) == EUNSUPPORTED

    B, K, Q = 8, 64, 3
    wneed = lib.kccot_weighted_sinkhorn_loss_dw_workspace_bytes(B, K)
    assert wneed >= lib.kccot_weighted_sinkhorn_loss_workspace_bytes(B, K) + 6 * B * 4 and wneed % 4 == 0
    assert lib.kccot_weighted_sinkhorn_loss_dw_workspace_bytes(0, K) == 0

    def lbwd(g=one, w_real=one, w_fake=one, B=B, T=4, eps=1.0, L=10, C3=one, dwr=one, dwf=one, ws=one, wsb=wneed):
        return lib.kccot_weighted_sinkhorn_loss_bwd_dw_f32(g, one, one, B, K, 1.0, one, one, one, one, T, 3, eps, L, w_real, w_fake,
                                                           C3, one, one, one, one, None, None, None, None, dwr, dwf, ws, wsb, None)

    for kw in ({"g": None}, {"w_real": None}, {"w_fake": None}, {"C3": None}, {"dwr": None}, {"dwf": None}, {"B": 0}, {"T": 0},
               {"eps": 0.0}, {"L": -1}):
        assert lbwd(**kw) == EINVAL, kw
    assert lbwd(wsb=wneed - 1) == EWORKSPACE and lbwd(ws=None) == EWORKSPACE and lbwd(B=1025, wsb=1 << 40) == EUNSUPPORTED

    need8, need130c = lib.kccot_sinkhorn_conditional_dw_workspace_bytes(2, 8), lib.kccot_sinkhorn_conditional_dw_workspace_bytes(2, 130)
    assert need8 >= lib.kccot_sinkhorn_conditional_workspace_bytes(2, 8) + 6 * 2 * 8 * 4 and need8 % 4 == 0
    assert need130c >= lib.kccot_sinkhorn_conditional_workspace_bytes(2, 130) + 6 * 2 * 130 * 4
    assert lib.kccot_sinkhorn_conditional_dw_workspace_bytes(0, 8) == 0 and lib.kccot_sinkhorn_conditional_dw_workspace_bytes(2, 1025) == 0

    def cbwd(g=one, C3=one, w=one, uh=one, vh=one, nits=one, Q=2, n=8, eps=1.0, L=10, dC=one, cost=one, dw=one, dom=one, ws=one,
             wsb=need8):
        return lib.kccot_sinkhorn_conditional_bwd_dw_f32(g, C3, w, None, uh, vh, nits, Q, n, eps, L, dC, cost, dw, dom, ws, wsb, None)

    for kw in ({"g": None}, {"C3": None}, {"w": None}, {"uh": None}, {"vh": None}, {"nits": None}, {"dC": None}, {"cost": None},
               {"dw": None}, {"Q": 0}, {"n": 0}, {"eps": 0.0}, {"eps": -1.0}, {"L": -1}):
        assert cbwd(**kw) == EINVAL, kw
    assert cbwd(n=1025) == EUNSUPPORTED
    assert cbwd(wsb=need8 - 1) == EWORKSPACE and cbwd(ws=None) == EWORKSPACE and cbwd(n=130, wsb=need130c - 1) == EWORKSPACE
    # a workspace that is enough for the backward WITHOUT dw is not enough here
    assert cbwd(wsb=lib.kccot_sinkhorn_conditional_workspace_bytes(2, 8)) == EWORKSPACE

    lneed = lib.kccot_conditional_sinkhorn_loss_dw_workspace_bytes(B, K, Q)
    assert lneed >= 3 * B * B * 4 + lib.kccot_sinkhorn_conditional_dw_workspace_bytes(Q, B)
    assert lneed >= lib.kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, Q)
    assert lib.kccot_conditional_sinkhorn_loss_dw_workspace_bytes(0, K, Q) == 0
    assert lib.kccot_conditional_sinkhorn_loss_dw_workspace_bytes(B, K, 0) == 0

    def clbwd(real=one, w=one, B=B, Q=Q, T=4, eps=1.0, L=10, C3=one, cost=one, dw=one, wsb=lneed):
        return lib.kccot_conditional_sinkhorn_loss_bwd_dw_f32(one, real, one, B, K, 1.0, one, one, one, one, T, 3, eps, L, w, None, Q,
                                                              C3, one, one, one, one, None, None, None, None, cost, dw, None, one,
                                                              wsb, None)

    for kw in ({"real": None}, {"w": None}, {"C3": None}, {"cost": None}, {"dw": None}, {"B": 0}, {"Q": 0}, {"T": 0}, {"eps": 0.0},
               {"L": -1}):
        assert clbwd(**kw) == EINVAL, kw
    assert clbwd(B=1025, wsb=1 << 40) == EUNSUPPORTED and clbwd(wsb=lneed - 1) == EWORKSPACE

    def wbwd(D=one, w=one, dw=one, Q=2, n=8, bw=1.0, dD=one, dbw=one):
        return lib.kccot_conditional_weights_bwd_f32(D, w, dw, Q, n, bw, dD, dbw, None)

    for kw in ({"D": None}, {"w": None}, {"dw": None}, {"dD": None}, {"dbw": None}, {"Q": 0}, {"n": 0}, {"bw": 0.0}, {"bw": -1.0},
               {"bw": float("nan")}):
        assert wbwd(**kw) == EINVAL, kw
    assert b"bandwidth" in lib.kccot_last_error()
    assert wbwd(n=1025) == EUNSUPPORTED

    def wdev(D=one, Q=2, n=8, bw=one, out=one):
        return lib.kccot_conditional_weights_dev_f32(D, Q, n, bw, out, None)

    def wbdev(D=one, w=one, dw=one, Q=2, n=8, bw=one, dD=one, dbw=one):
        return lib.kccot_conditional_weights_bwd_dev_f32(D, w, dw, Q, n, bw, dD, dbw, None)

    for kw in ({"D": None}, {"bw": None}, {"out": None}, {"Q": 0}, {"n": 0}):
        assert wdev(**kw) == EINVAL, kw
    for kw in ({"D": None}, {"w": None}, {"dw": None}, {"bw": None}, {"dD": None}, {"dbw": None}, {"Q": 0}, {"n": 0}):
        assert wbdev(**kw) == EINVAL, kw
    assert wdev(n=1025) == EUNSUPPORTED and wbdev(n=1025) == EUNSUPPORTED


# ================================================================ 5. the Python surface
def test_python_surface():
    from kccotgan_amd import gan_utils as g, _lib
    assert "compute_kernel_conditional_sinkhorn_loss" in g.__all__
    p = inspect.signature(g.compute_kernel_conditional_sinkhorn_loss).parameters
    assert list(p) == ["f_real", "f_fake", "scaling_coef", "sinkhorn_eps", "sinkhorn_l", "h_fake", "m_real", "h_real", "m_fake",
                       "context", "bandwidth", "queries", "query_weights", "video"]
    assert p["queries"].default is None and p["query_weights"].default is None and p["video"].default is True
    x, f, w = torch.zeros(2, 3, 4), torch.zeros(2, 3, 2), torch.full((3, 2), 0.5)
    with pytest.raises(_lib.KccotError):                       # well-formed, but there is no CPU path
        g.compute_kernel_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, x, 1.0, video=False)
    with pytest.raises(_lib.KccotError):                       # ... also when the new leaves want a gradient
        g.compute_kernel_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, x.clone().requires_grad_(True),
                                                   torch.tensor(1.0, requires_grad=True), video=False)
    for bw in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            g.compute_kernel_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, x, bw, video=False)
    with pytest.raises(ValueError):
        g.compute_kernel_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, x, torch.ones(2), video=False)
    with pytest.raises(NotImplementedError):
        g.compute_kernel_conditional_sinkhorn_loss(x.clone().requires_grad_(True), x, 1.0, 1.0, 10, f, f, f, f, x, 1.0, video=False)
    # the weighted wrappers no longer refuse a weight that requires a gradient: on the CPU they now fail for want of a device
    wv = torch.full((2,), 0.5, requires_grad=True)
    with pytest.raises(_lib.KccotError):
        g.compute_weighted_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, wv, wv, video=False)
    # the existing conditional pair still refuses, and says where to go
    with pytest.raises(NotImplementedError, match="compute_kernel_conditional_sinkhorn_loss"):
        g.kernel_conditional_weights(x.clone().requires_grad_(True), 1.0)
    with pytest.raises(NotImplementedError, match="compute_kernel_conditional_sinkhorn_loss"):
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w.clone().requires_grad_(True), video=False)
    with pytest.raises(NotImplementedError, match="compute_kernel_conditional_sinkhorn_loss"):
        g.compute_conditional_sinkhorn_loss(x, x, 1.0, 1.0, 10, f, f, f, f, w, torch.ones(3).requires_grad_(True), video=False)
