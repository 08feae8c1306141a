"""Bounds tests of the C ABI: every compute entry point of include/kccot.h, called through ctypes on guarded buffers
(tests/abi_guard.py), at the shapes where kernels go wrong (dispatch edges, ragged tails, tiny frames).  Each case asserts
  (a) the guard zones of every output and of the workspace are intact;
  (b) every input is unchanged, bit for bit;
  (c) every element the header says is written no longer holds the NaN pre-fill, and every element outside that region does;
  (d) the outputs are bit-identical with the workspace full of sentinel and zero-filled (no state carried in it);
  (e) `ticket` is zero after every call that takes one;
  (f) the values agree with the fp64 oracles, at the tolerance the existing tests use for that entry point.
The workspace is exactly the size its query returns.  Selected cases run again with every fp32 argument at a 4-byte offset
from its 16-byte alignment (the vector-width fast paths must test the alignment and fall back)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_guard as ag
from oracle import gan_utils_np as o
from oracle import gan_utils_torch as ot

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, I32, F64 = torch.float32, torch.int32, torch.float64
THRESH = o.THRESH
GRAD_TOL = 2.5e-5            # test_gpu_parity.py GRAD_TOL_FLOOR: gradients, relative to max|grad| (well-conditioned inputs)


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def _defaults(L):
    defaults = {k: L.get_option(k) for k in L.option_names()}
    yield
    for k, v in defaults.items():
        L.set_option(k, v)


def ws_query(L, name, *a):
    return int(getattr(L.lib, name)(*a))


def guarded_call(L, sym, argspec, ins, outs, ws_bytes=0, offset=0, regions=None, ws_keep=None, zero_in=()):
    """Run `sym` twice -- workspace full of sentinel, then zero-filled -- on guarded copies of `ins` (name -> tensor) and
    guarded outputs `outs` (name -> (shape, dtype)), checking (a)-(e).  argspec: the argument list, "@name" = pointer of
    that buffer ("@ws" the workspace, "@ws_bytes" its size).  offset: fp32 buffers start 4 bytes off their alignment.
    regions(res) -> {name: bool mask of the elements that must be written} (default: all).  ws_keep = (byte offset, bytes,
    uint8 tensor): a span of the workspace that is restored after the poisoning (the documented Gram-sums hand-over).
    zero_in: outputs that must be zero on entry (tickets).  Returns the outputs of the second run."""
    fn = getattr(L.lib, sym)
    gi = {k: ag.guarded_input(k, v.contiguous(), offset if v.dtype == F32 else 0) for k, v in ins.items()}
    snap = {k: g.payload().clone() for k, g in gi.items()}
    runs = []
    for ws_mode in ("workspace", "zero"):
        go = {k: ag.guarded((int(np.prod(s)) if len(s) else 1) * torch.empty((), dtype=d).element_size(),
                            "zero" if k in zero_in else "output", k, offset if d == F32 else 0) for k, (s, d) in outs.items()}
        gw = ag.guarded(ws_bytes, ws_mode, "workspace") if ws_bytes else None
        if ws_keep is not None:
            off, nb, data = ws_keep
            gw.payload()[off:off + nb].copy_(data)
        ptrs = {k: g.ptr for k, g in list(gi.items()) + list(go.items())}
        ptrs["ws"], ptrs["ws_bytes"] = (gw.ptr if gw else None), ws_bytes
        args = [ptrs[a[1:]] if isinstance(a, str) and a.startswith("@") else a for a in argspec]
        rc = fn(*args)
        torch.cuda.synchronize()
        assert rc == 0, "%s returned %d: %s" % (sym, rc, L.lib.kccot_last_error().decode())
        bad = [m for m in (g.verify() for g in list(gi.values()) + list(go.values()) + ([gw] if gw else [])) if m]
        assert not bad, "%s (%s workspace): guard zone damaged: %s" % (sym, ws_mode, "; ".join(bad))
        for k, g in gi.items():
            assert torch.equal(g.payload(), snap[k]), "%s wrote its input %s" % (sym, k)
        res = {k: go[k].view(d, tuple(s)).clone() for k, (s, d) in outs.items()}
        for k in zero_in:
            assert int(res[k].reshape(-1)[0]) == 0, "%s left %s = %d" % (sym, k, int(res[k].reshape(-1)[0]))
        runs.append(res)
    a, b = runs
    for k in outs:
        assert ag.same_bits(a[k], b[k]), "%s: output %s depends on the workspace contents" % (sym, k)
    want = regions(b) if regions else {}
    for k in outs:
        if k in zero_in:
            continue
        uw = ag.unwritten(b[k])
        m = want.get(k)
        if m is None:
            assert not bool(uw.any()), "%s: %d of %d elements of %s never written" % (sym, int(uw.sum()), uw.numel(), k)
            continue
        must, may = (m, m) if torch.is_tensor(m) else m        # (elements that must be written, elements that may be)
        must, may = must.to(uw.device), may.to(uw.device)
        assert not bool((uw & must).any()), "%s: %d elements of %s inside the written region never written" % (sym, int((uw & must).sum()), k)
        assert bool(uw[~may].all()), "%s: %d elements of %s outside the written region were written" % (sym, int((~uw & ~may).sum()), k)
    return b


def close(got, ref, atol_rel, what, rtol=0.0, atol=None):
    got = got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = ref.detach().cpu().double().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    tol = atol if atol is not None else atol_rel * max(float(np.abs(ref).max()), 1e-30)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=tol, err_msg=what)


def rng_inputs(B, K, T, J, seed, near=True):
    g = torch.Generator().manual_seed(seed)
    real = torch.rand(B, K, generator=g)
    fake = (real + 0.1 * torch.randn(B, K, generator=g)).clamp(0, 1) if near else torch.rand(B, K, generator=g)
    f = {k: torch.rand(B, T, J, generator=g) for k in ("h_fake", "h_real", "m_real", "m_fake")}
    return real, fake, f


def oracle_cost3(real, fake, f, sc):
    r, y = real.double()[:, None], fake.double()[:, None]
    d = {k: v.double() for k, v in f.items()}
    return torch.stack([ot.modified_cost(r, y, d["h_fake"], d["m_real"], sc), ot.modified_cost(r, r, d["h_real"], d["m_real"], sc),
                        ot.modified_cost(y, y, d["h_fake"], d["m_fake"], sc)])


def hist_regions(nprob, L_, n, nits, names=("u_hist", "v_hist")):
    """Rows of the executed iterations must be written; rows at and past the reference's count never are (in between: the
    iterations the exact periodic-state shortcut skipped, which the solver may fill in)."""
    nits = nits.reshape(-1).cpu()
    must = torch.zeros(nprob, max(L_, 1), n, dtype=torch.bool)
    may = must.clone()
    for p in range(nprob):
        must[p, :int(nits[nprob + p])] = True
        may[p, :int(nits[p])] = True
    return {k: (must, may) for k in names}


# ---------------------------------------------------------------- pairwise cost
@pytest.mark.parametrize("Bx,By,K,flags,feat", [(1, 1, 1, 0, False), (7, 63, 13, 0, True), (65, 8, 255, 2, True),
                                                 (64, 64, 257, 0, True), (63, 129, 64, 2, False), (64, 64, 260, 4, True),
                                                 (8, 8, 256, 4, False), (129, 127, 37, 0, True)])
def test_pairwise_cost(L, Bx, By, K, flags, feat):
    T, J, sc = 3, 4, 0.7
    g = torch.Generator().manual_seed(Bx * 7 + By + K)
    x, y = torch.rand(Bx, K, generator=g), torch.rand(By, K, generator=g)
    h, M = (torch.rand(Bx, T, J, generator=g), torch.rand(By, T, J, generator=g)) if feat else (None, None)
    ins = {"x": x.to(DEV), "y": y.to(DEV)}
    if feat:
        ins.update(h=h.to(DEV), M=M.to(DEV))
    ws = ws_query(L, "kccot_pairwise_cost_workspace_bytes", Bx, By, K)
    res = guarded_call(L, "kccot_pairwise_cost_f32", ["@x", "@y", Bx, By, K, sc, "@h" if feat else None, "@M" if feat else None,
                                                      None, None, T, J, flags, "@C_out", "@ws", "@ws_bytes", None],
                       ins, {"C_out": ((Bx, By), F32)}, ws)
    ref = ot.cost_xy(x.double()[:, None], y.double()[:, None], sc)
    if feat:
        ref = ref + ot.causal_term(h.double(), M.double(), sc)
    close(res["C_out"], ref, 1e-5, "C_out")


# cost3: B at every tile edge, K ragged / around 256, each path forced
COST3 = [(1, 5, {}), (7, 255, {}), (8, 256, {}), (63, 257, {}), (64, 260, {}), (65, 253, {}), (127, 64, {}), (128, 256, {}),
         (129, 260, {}), (256, 512, {}), (257, 36, {}), (64, 256, "mfma"), (8, 260, "mfma"), (128, 260, "direct"),
         (128, 512, dict(cost_tiled=0)), (256, 512, dict(cost_tile256=0)), (192, 256, dict(cost_blocked=0)),
         (128, 256, dict(gram_f32=1))]


@pytest.mark.parametrize("B,K,path", COST3)
def test_cost3(L, B, K, path, offset=0):
    T, J, sc = 4, 3, 1.0 / K
    real, fake, f = rng_inputs(B, K, T, J, B + K)
    flags = {"mfma": L.COST_FORCE_MFMA, "direct": L.COST_FORCE_DIRECT}.get(path, 0) if isinstance(path, str) else 0
    ins = {"real": real.to(DEV), "fake": fake.to(DEV), **{k: v.to(DEV) for k, v in f.items()}}
    ws = ws_query(L, "kccot_pairwise_cost3_workspace_bytes", B, K)
    spec = ["@real", "@fake", B, K, sc, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, flags, "@C3", "@ws", "@ws_bytes", None]
    with L.options(**(path if isinstance(path, dict) else {})):
        res = guarded_call(L, "kccot_pairwise_cost3_f32", spec, ins, {"C3": ((3, B, B), F32)}, ws, offset=offset)
    ref = oracle_cost3(real, fake, f, sc)
    for p in range(3):
        close(res["C3"][p], ref[p], 1e-5, "C3[%d]" % p)
    return res


@pytest.mark.parametrize("B,K", [(7, 255), (64, 260), (129, 253)])
def test_cost3_at_a_4_byte_offset(L, B, K):
    test_cost3(L, B, K, {}, offset=4)


@pytest.mark.parametrize("B", [64, 128, 256])
def test_cost3_gram_sums_split(L, B):
    """GRAM_SUMS_ONLY then FROM_GRAM_SUMS: the second call's workspace is poisoned everywhere except the documented span."""
    import ctypes
    K, T, J, sc = 512, 3, 2, 1.0 / 512
    real, fake, f = rng_inputs(B, K, T, J, B)
    ins = {"real": real.to(DEV), "fake": fake.to(DEV), **{k: v.to(DEV) for k, v in f.items()}}
    ws = ws_query(L, "kccot_pairwise_cost3_workspace_bytes", B, K)
    off, nd = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lib.kccot_pairwise_cost3_gram_sums_span(B, K, ctypes.byref(off), ctypes.byref(nd)) == 0 and nd.value > 0
    gw = ag.guarded(ws, "workspace", "workspace")
    gi = {k: ag.guarded_input(k, v) for k, v in ins.items()}
    c3 = ag.guarded(3 * B * B * 4, "output", "C3")
    p = {k: g.ptr for k, g in gi.items()}
    assert L.lib.kccot_pairwise_cost3_f32(p["real"], p["fake"], B, K, sc, p["h_fake"], p["h_real"], p["m_real"], p["m_fake"], T, J,
                                          L.COST_GRAM_SUMS_ONLY, c3.ptr, gw.ptr, ws, None) == 0
    torch.cuda.synchronize()
    assert gw.verify() is None and c3.verify() is None
    assert bool(ag.unwritten(c3.view(F32, (3, B, B))).all()), "GRAM_SUMS_ONLY wrote C3"
    span = gw.payload()[off.value:off.value + 8 * nd.value].clone()
    spec = ["@real", "@fake", B, K, sc, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, L.COST_FROM_GRAM_SUMS, "@C3", "@ws",
            "@ws_bytes", None]
    res = guarded_call(L, "kccot_pairwise_cost3_f32", spec, ins,
                       {"C3": ((3, B, B), F32)}, ws, ws_keep=(off.value, 8 * nd.value, span))
    ref = oracle_cost3(real, fake, f, sc)
    for q in range(3):
        close(res["C3"][q], ref[q], 1e-5, "C3[%d]" % q)


@pytest.mark.parametrize("B,K,rb,rc", [(7, 13, 1, 5), (65, 257, 3, 61), (129, 64, 63, 66), (257, 36, 250, 7)])
def test_cost3_rows(L, B, K, rb, rc):
    T, J, sc = 3, 5, 1.0 / K
    real, fake, f = rng_inputs(B, K, T, J, B * 3 + rb)
    ins = {"real": real.to(DEV), "fake": fake.to(DEV), **{k: v.to(DEV) for k, v in f.items()}}
    ws = ws_query(L, "kccot_pairwise_cost3_rows_workspace_bytes", rc, B, K)
    res = guarded_call(L, "kccot_pairwise_cost3_rows_f32", ["@real", "@fake", B, K, sc, "@h_fake", "@h_real", "@m_real", "@m_fake",
                                                            T, J, rb, rc, "@C3_rows", "@ws", "@ws_bytes", None],
                       ins, {"C3_rows": ((3, rc, B), F32)}, ws)
    ref = oracle_cost3(real, fake, f, sc)[:, rb:rb + rc]
    for q in range(3):
        close(res["C3_rows"][q], ref[q], 1e-5, "C3_rows[%d]" % q)


@pytest.mark.parametrize("rc,B,K,rb", [(32, 128, 260, 32), (64, 256, 512, 192)])
def test_rows_gram(L, rc, B, K, rb):
    """Row norms, the one-call Gram row block, and the two-stage form (sums, then the block from the sums)."""
    assert L.lib.kccot_pairwise_cost3_rows_gram_supported(rc, B, K) == 1
    T, J, sc = 3, 4, 1.0 / K
    real, fake, f = rng_inputs(B, K, T, J, rc + B)
    ins = {"real": real.to(DEV), "fake": fake.to(DEV)}
    feats = {k: v.to(DEV) for k, v in f.items()}
    wsn = ws_query(L, "kccot_row_norms_workspace_bytes", B)
    norms = guarded_call(L, "kccot_row_norms_f64", ["@real", "@fake", B, K, "@norms_out", "@ws", "@ws_bytes", None], ins,
                         {"norms_out": ((B, 3), F64)}, wsn)["norms_out"]
    r, e = real.double(), (fake - real).double()
    close(norms, torch.stack([(r * r).sum(1), (e * e).sum(1), (r * e).sum(1)], 1), 1e-6, "norms")
    ref = oracle_cost3(real, fake, f, sc)[:, rb:rb + rc]
    wsg = ws_query(L, "kccot_pairwise_cost3_rows_gram_workspace_bytes", rc, B, K)
    res = guarded_call(L, "kccot_pairwise_cost3_rows_gram_f32",
                       ["@real", "@fake", B, K, sc, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, rb, rc, "@norms", "@C3_rows",
                        "@ws", "@ws_bytes", None], dict(ins, norms=norms, **feats), {"C3_rows": ((3, rc, B), F32)}, wsg)
    for q in range(3):
        close(res["C3_rows"][q], ref[q], 1e-5, "gram C3_rows[%d]" % q)
    ns = int(L.lib.kccot_pairwise_cost3_rows_gram_sums_count(rc, B))
    gsum = guarded_call(L, "kccot_pairwise_cost3_rows_gram_sums_f64",
                        ["@real", "@fake", B, K, rb, rc, "@gsum", 0, "@ws", "@ws_bytes", None], ins, {"gsum": ((ns,), F64)}, wsg)["gsum"]
    res2 = guarded_call(L, "kccot_pairwise_cost3_rows_gram_from_sums_f32",
                        ["@gsum", B, sc, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, rb, rc, "@norms", "@C3_rows", None],
                        dict(feats, gsum=gsum, norms=norms), {"C3_rows": ((3, rc, B), F32)})
    for q in range(3):
        close(res2["C3_rows"][q], ref[q], 1e-5, "from_sums C3_rows[%d]" % q)


# ---------------------------------------------------------------- cost backward
def cost3_grad_oracle(real, fake, f, g3, sc, rows=None):
    y = fake.double().requires_grad_(True)
    d = {k: v.double().requires_grad_(True) for k, v in f.items()}
    C = oracle_cost3(real, y, d, sc)
    (C * g3.double()).sum().backward()
    out = {"dfake": y.grad, "dh_fake": d["h_fake"].grad, "dh_real": d["h_real"].grad, "dm_real": d["m_real"].grad,
           "dm_fake": d["m_fake"].grad}
    if rows:
        out = {k: v[rows[0]:rows[0] + rows[1]] for k, v in out.items()}
    return out


COST3_BWD = [(1, 5, None, {}), (7, 13, None, {}), (8, 256, None, {}), (8, 260, None, dict(apply_one_launch=0)),
             (40, 2052, None, {}), (63, 257, None, {}), (64, 4096, None, {}), (64, 260, None, dict(apply_one_launch=0)),
             (65, 255, None, {}), (127, 64, None, {}), (128, 260, None, {}), (129, 36, None, {}), (256, 512, None, {}),
             (256, 512, None, dict(apply_m256=0)), (257, 37, None, {}), (64, 256, None, dict(apply_f32=1)),
             (65, 257, (3, 60), {}), (128, 256, (32, 64), {}), (129, 260, (64, 65), {})]


@pytest.mark.parametrize("B,K,rows,opts", COST3_BWD)
def test_cost3_bwd(L, B, K, rows, opts, offset=0, scaled=False):
    T, J, sc = 3, 4, 1.0 / K
    real, fake, f = rng_inputs(B, K, T, J, B + 3 * K)
    g3 = torch.randn(3, B, B, generator=torch.Generator().manual_seed(B))
    rb, rc = rows or (0, B)
    ins = {"g3": g3.to(DEV), "real": real.to(DEV), "fake": fake.to(DEV), **{k: v.to(DEV) for k, v in f.items()}}
    outs = {"dfake": ((rc, K), F32), **{k: ((rc, T, J), F32) for k in ("dh_fake", "dh_real", "dm_real", "dm_fake")}}
    tail = ["@dfake", "@dh_fake", "@dh_real", "@dm_real", "@dm_fake", "@ws", "@ws_bytes", None]
    mid = ["@real", "@fake", B, K, sc, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J]
    ws = ws_query(L, "kccot_pairwise_cost3_bwd_workspace_bytes", B, K)
    with L.options(**opts):
        if rows:
            res = guarded_call(L, "kccot_pairwise_cost3_bwd_rows_f32", ["@g3"] + mid + [rb, rc] + tail, ins, outs, ws, offset=offset)
        elif scaled:
            ins["gscale"] = torch.tensor([-1.75], device=DEV)
            res = guarded_call(L, "kccot_pairwise_cost3_bwd_scaled_f32", ["@g3", "@gscale"] + mid + tail, ins, outs, ws, offset=offset)
        else:
            res = guarded_call(L, "kccot_pairwise_cost3_bwd_f32", ["@g3"] + mid + tail, ins, outs, ws, offset=offset)
    ref = cost3_grad_oracle(real, fake, f, g3 * (-1.75 if scaled else 1.0), sc, rows)
    for k in outs:
        close(res[k], ref[k], GRAD_TOL, k)
    return res


@pytest.mark.parametrize("B,K", [(8, 256), (64, 260), (65, 255), (129, 36)])
def test_cost3_bwd_scaled(L, B, K):
    test_cost3_bwd(L, B, K, None, {}, scaled=True)


@pytest.mark.parametrize("B,K,rows", [(7, 13, None), (64, 260, None), (65, 257, (3, 60)), (128, 260, None)])
def test_cost3_bwd_at_a_4_byte_offset(L, B, K, rows):
    test_cost3_bwd(L, B, K, rows, {}, offset=4)


@pytest.mark.parametrize("B,K", [(8, 256), (64, 4096), (40, 2052)])
def test_one_launch_backward_falls_back_on_a_misaligned_dC(L, B, K):
    """The one-launch backward reads dC3 with 16-byte loads: with dC3 at a 4-byte offset it must take the two-launch form
    -- dfake bit-identical to apply_one_launch = 0 (the two forms differ by up to 4e-6 of max|dfake| otherwise)."""
    T, J, sc = 3, 4, 1.0 / K
    real, fake, f = rng_inputs(B, K, T, J, B + K)
    g3 = torch.randn(3, B, B, generator=torch.Generator().manual_seed(B + 1)).to(DEV)
    ws = ws_query(L, "kccot_pairwise_cost3_bwd_workspace_bytes", B, K)
    ins = {"real": real.to(DEV), "fake": fake.to(DEV), **{k: v.to(DEV) for k, v in f.items()}}
    outs = {"dfake": ((B, K), F32), **{k: ((B, T, J), F32) for k in ("dh_fake", "dh_real", "dm_real", "dm_fake")}}
    spec = ["@g3", "@real", "@fake", B, K, sc, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, "@dfake", "@dh_fake", "@dh_real",
            "@dm_real", "@dm_fake", "@ws", "@ws_bytes", None]
    with L.options(apply_one_launch=0):
        two = guarded_call(L, "kccot_pairwise_cost3_bwd_f32", spec, dict(ins, g3=g3), outs, ws)
    gi = ag.guarded_input("g3", g3, offset=4)
    gin = {k: ag.guarded_input(k, v) for k, v in ins.items()}
    go = {k: ag.guarded(int(np.prod(s)) * 4, "output", k) for k, (s, d) in outs.items()}
    gw = ag.guarded(ws, "workspace", "workspace")
    p = {k: g.ptr for k, g in list(gin.items()) + list(go.items())}
    rc = L.lib.kccot_pairwise_cost3_bwd_f32(gi.ptr, p["real"], p["fake"], B, K, sc, p["h_fake"], p["h_real"], p["m_real"], p["m_fake"],
                                            T, J, p["dfake"], p["dh_fake"], p["dh_real"], p["dm_real"], p["dm_fake"], gw.ptr, ws, None)
    torch.cuda.synchronize()
    assert rc == 0
    bad = [m for m in (g.verify() for g in [gi, gw] + list(gin.values()) + list(go.values())) if m]
    assert not bad, bad
    for k, (s, d) in outs.items():
        assert ag.same_bits(go[k].view(d, s), two[k]), "%s with dC3 at a 4-byte offset differs from the two-launch form" % k


@pytest.mark.parametrize("Bx,By,K,same", [(1, 1, 1, False), (7, 65, 13, False), (64, 64, 256, False), (65, 65, 257, True),
                                          (129, 8, 260, False), (128, 128, 64, True)])
def test_pairwise_cost_bwd(L, Bx, By, K, same):
    T, J, sc = 3, 2, 0.5 / K
    g = torch.Generator().manual_seed(Bx + By * 3 + K)
    x = torch.rand(Bx, K, generator=g)
    y = x if same else torch.rand(By, K, generator=g)
    h, M = torch.rand(Bx, T, J, generator=g), torch.rand(By, T, J, generator=g)
    gC = torch.randn(Bx, By, generator=g)
    ins = {"g": gC.to(DEV), "x": x.to(DEV), "h": h.to(DEV), "M": M.to(DEV)}
    if not same:
        ins["y"] = y.to(DEV)
    outs = {"dx": ((Bx, K), F32), "dh": ((Bx, T, J), F32), "dM": ((By, T, J), F32)}
    if not same:
        outs["dy"] = ((By, K), F32)
    ws = ws_query(L, "kccot_pairwise_cost_bwd_workspace_bytes", Bx, By)
    res = guarded_call(L, "kccot_pairwise_cost_bwd_f32", ["@g", "@x", "@x" if same else "@y", Bx, By, K, sc, "@h", "@M", T, J, L.COST_SAME if same else 0,
                                                          "@dx", None if same else "@dy", "@dh", "@dM", "@ws", "@ws_bytes", None],
                       ins, outs, ws)
    xd, hd, Md = x.double().requires_grad_(True), h.double().requires_grad_(True), M.double().requires_grad_(True)
    yd = xd if same else y.double().requires_grad_(True)
    C = ot.cost_xy(xd[:, None], yd[:, None], sc) + ot.causal_term(hd, Md, sc)
    (C * gC.double()).sum().backward()
    close(res["dx"], xd.grad, GRAD_TOL, "dx")
    if not same:
        close(res["dy"], yd.grad, GRAD_TOL, "dy")
    close(res["dh"], hd.grad, GRAD_TOL, "dh")
    close(res["dM"], Md.grad, GRAD_TOL, "dM")


# ---------------------------------------------------------------- Sinkhorn
def nits_ok(got, a, b):
    lo, hi = min(a, b), max(a, b)
    return lo - (hi - lo) <= got <= hi + (hi - lo)


def cost_matrix(nprob, n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(nprob, n, 6, generator=g)
    y = (x + 0.3 * torch.rand(nprob, n, 6, generator=g))
    return (scale * ((x[:, :, None] - y[:, None]) ** 2).sum(-1)).float()


def sinkhorn_oracle(C, eps, nits, grad=None):
    """fp64 value (and gradient) of the solve unrolled over exactly `nits` iterations (the reference's count)."""
    Cd = C.double().requires_grad_(grad is not None)
    cost = ot.sinkhorn_from_cost(Cd, eps, nits, nits)[0]
    if grad is None:
        return float(cost), None
    (cost * grad).backward()
    return float(cost), Cd.grad


SINKHORN = [(1, 1, 10, 10, {}), (1, 2, 0, 0, {}), (3, 33, 1, 1, {}), (1, 64, 60, 5, {}), (4, 65, 40, 10, {}),
            (1, 128, 30, 30, {}), (3, 129, 25, 5, {}), (1, 256, 20, 10, {}), (4, 257, 30, 3, {}), (1, 1024, 12, 12, {}),
            (3, 256, 25, 5, dict(sinkhorn_coop=0)), (3, 512, 10, 5, dict(sinkhorn_coop_max_wg=8)),
            (1, 64, 300, 300, dict(sinkhorn_shortcut=1)), (1, 64, 300, 300, dict(sinkhorn_shortcut=0))]


@pytest.mark.parametrize("nprob,n,L_,Lmin,opts", SINKHORN)
def test_sinkhorn(L, nprob, n, L_, Lmin, opts, offset=0):
    eps = 0.5
    C = cost_matrix(nprob, n, n * 10 + nprob, 0.1)
    ws = ws_query(L, "kccot_sinkhorn_workspace_bytes", nprob, n)
    outs = {"u_hist": ((nprob, max(L_, 1), n), F32), "v_hist": ((nprob, max(L_, 1), n), F32), "cost_out": ((nprob,), F32),
            "nits_out": ((2 * nprob,), I32), "pi_out": ((nprob, n, n), F32)}
    with L.options(**opts):
        fwd = guarded_call(L, "kccot_sinkhorn_fwd_f32", ["@C", nprob, n, eps, L_, Lmin, THRESH, L.STOP_COUNT, "@u_hist", "@v_hist",
                                                        "@cost_out", "@nits_out", "@pi_out", "@ws", "@ws_bytes", None],
                           {"C": C.to(DEV)}, outs, ws, offset=offset,
                           regions=lambda r: hist_regions(nprob, L_, n, r["nits_out"]))
        gcost = torch.randn(nprob, generator=torch.Generator().manual_seed(n))
        bwd = guarded_call(L, "kccot_sinkhorn_bwd_f32", ["@C", "@u_hist", "@v_hist", "@nits", nprob, n, eps, L_, "@gcost", "@dC_out",
                                                        "@ws", "@ws_bytes", None],
                           {"C": C.to(DEV), "u_hist": fwd["u_hist"], "v_hist": fwd["v_hist"], "nits": fwd["nits_out"],
                            "gcost": gcost.to(DEV)}, {"dC_out": ((nprob, n, n), F32)}, ws, offset=offset)
    nits = fwd["nits_out"].cpu()
    for p in range(nprob):
        a = o.sinkhorn_from_cost(C[p].numpy(), eps, L_, Lmin, dtype=np.float32)[1]
        b = o.sinkhorn_from_cost(C[p].numpy(), eps, L_, Lmin, dtype=np.float64)[1]
        assert nits_ok(int(nits[p]), a, b), (p, int(nits[p]), a, b)
        assert 0 <= int(nits[nprob + p]) <= int(nits[p])
        ref, gref = sinkhorn_oracle(C[p], eps, int(nits[p]), float(gcost[p]))
        assert abs(float(fwd["cost_out"][p]) - ref) <= 1e-4 * abs(ref), (p, float(fwd["cost_out"][p]), ref)
        close(bwd["dC_out"][p], gref, GRAD_TOL, "dC[%d]" % p)


@pytest.mark.parametrize("nprob,n", [(3, 33), (1, 257), (3, 1024)])
def test_sinkhorn_at_a_4_byte_offset(L, nprob, n):
    test_sinkhorn(L, nprob, n, 12, 3, {}, offset=4)


@pytest.mark.parametrize("n,L_,Lmin,fused", [(1, 5, 5, True), (2, 0, 0, False), (33, 1, 1, True), (64, 40, 5, True),
                                             (64, 40, 5, False), (65, 30, 10, False), (128, 20, 20, False)])
def test_divergence(L, n, L_, Lmin, fused):
    eps = 0.6
    C3 = cost_matrix(3, n, n + L_, 0.1)
    ws = ws_query(L, "kccot_sinkhorn_workspace_bytes", 3, n)
    gloss = torch.tensor([1.3])
    if fused:
        assert L.lib.kccot_sinkhorn_fused_eligible(n, L_) == 1
        res = guarded_call(L, "kccot_sinkhorn_divergence_fused_f32", ["@C3", n, eps, L_, Lmin, THRESH, "@cost3_out", "@nits_out",
                                                                      "@loss_out", "@ticket", "@dC3_unit", None],
                           {"C3": C3.to(DEV)}, {"cost3_out": ((3,), F32), "nits_out": ((6,), I32), "loss_out": ((1,), F32),
                                                "ticket": ((1,), I32), "dC3_unit": ((3, n, n), F32)}, zero_in=("ticket",))
        dC3, gl = res["dC3_unit"], 1.0
    else:
        res = guarded_call(L, "kccot_sinkhorn_divergence_fwd_f32", ["@C3", n, eps, L_, Lmin, THRESH, "@u_hist", "@v_hist", "@cost3_out",
                                                                    "@nits_out", "@loss_out", "@ticket", "@ws", "@ws_bytes", None],
                           {"C3": C3.to(DEV)}, {"u_hist": ((3, max(L_, 1), n), F32), "v_hist": ((3, max(L_, 1), n), F32),
                                                "cost3_out": ((3,), F32), "nits_out": ((6,), I32), "loss_out": ((1,), F32),
                                                "ticket": ((1,), I32)}, ws, zero_in=("ticket",),
                           regions=lambda r: hist_regions(3, L_, n, r["nits_out"]))
        dC3 = guarded_call(L, "kccot_sinkhorn_divergence_bwd_f32", ["@C3", "@u_hist", "@v_hist", "@nits", n, eps, L_, "@gloss",
                                                                    "@dC3_out", "@ws", "@ws_bytes", None],
                           {"C3": C3.to(DEV), "u_hist": res["u_hist"], "v_hist": res["v_hist"], "nits": res["nits_out"],
                            "gloss": gloss.to(DEV)}, {"dC3_out": ((3, n, n), F32)}, ws)["dC3_out"]
        gl = float(gloss[0])
    nits = res["nits_out"].cpu()
    refs = []
    for p, w in enumerate((2.0, -1.0, -1.0)):
        ref, gref = sinkhorn_oracle(C3[p], eps, int(nits[p]), w * gl)
        refs.append(ref)
        assert abs(float(res["cost3_out"][p]) - ref) <= 1e-4 * abs(ref)
        close(dC3[p], gref, GRAD_TOL, "dC3[%d]" % p)
    want = 2 * refs[0] - refs[1] - refs[2]
    assert abs(float(res["loss_out"][0]) - want) <= 1e-4 * max(abs(want), abs(refs[0]))


def test_mixed_divergence(L):
    cost3 = torch.tensor([1.5, 0.25, -3.0])
    loss = guarded_call(L, "kccot_mixed_divergence_fwd_f32", ["@cost3", "@loss_out", None], {"cost3": cost3.to(DEV)},
                        {"loss_out": ((1,), F32)})["loss_out"]
    assert float(loss[0]) == np.float32(2 * 1.5 - 0.25 + 3.0)
    g = guarded_call(L, "kccot_mixed_divergence_bwd_f32", ["@gloss", "@gcost3_out", None], {"gloss": torch.tensor([0.5], device=DEV)},
                     {"gcost3_out": ((3,), F32)})["gcost3_out"]
    assert g.cpu().tolist() == [1.0, -0.5, -0.5]


# ---------------------------------------------------------------- losses
def loss_oracle(kind, real, fake, f, sc, eps, nits, gl, realp=None, fakep=None, fp=None):
    """fp64 loss and gradients (fake / F and the features), each solve unrolled over the kernel's reference count."""
    y = fake.double().requires_grad_(True)
    d = {k: v.double().requires_grad_(True) for k, v in f.items()}
    x = real.double()[:, None]
    yy = y[:, None]
    W = lambda C, p: ot.sinkhorn_from_cost(C, eps, int(nits[p]), int(nits[p]))[0]
    l2, caus = ot.cost_xy, ot.causal_term
    if kind == "one":
        Cs = [l2(x, yy, sc) + caus(d["h_fake"], d["m_real"], sc), l2(x, x, sc) + caus(d["h_real"], d["m_real"], sc),
              l2(yy, yy, sc) + caus(d["h_fake"], d["m_fake"], sc)]
        loss = 2 * W(Cs[0], 0) - W(Cs[1], 1) - W(Cs[2], 2)
    elif kind == "bicausal":
        Cs = [l2(x, yy, sc) + caus(d["h_fake"], d["m_real"], sc) + caus(d["h_real"], d["m_fake"], sc),
              l2(x, x, sc) + 2 * caus(d["h_real"], d["m_real"], sc), l2(yy, yy, sc) + 2 * caus(d["h_fake"], d["m_fake"], sc)]
        loss = 2 * W(Cs[0], 0) - W(Cs[1], 1) - W(Cs[2], 2)
    else:
        B = real.shape[0] // 2
        xs, ys = x[:B], yy[:B]
        xp, yp = x[B:], yy[B:]
        Cs = [l2(xs, ys, sc) + caus(d["h_fake"], d["m_real"], sc), l2(xp, yp, sc) + caus(d["h_fake_p"], d["m_real_p"], sc),
              l2(xs, xp, sc) + caus(d["h_real_p"], d["m_real"], sc), l2(ys, yp, sc) + caus(d["h_fake_p"], d["m_fake"], sc)]
        loss = W(Cs[0], 0) + W(Cs[1], 1) - W(Cs[2], 2) - W(Cs[3], 3)
    (loss * gl).backward()
    grads = {"dF" if kind == "mixed" else "dfake": y.grad, **{"d" + k: v.grad for k, v in d.items()}}
    return float(loss), [c.detach() for c in Cs], grads


LOSS = [(8, 260, True), (8, 260, False), (40, 255, True), (64, 512, True), (64, 512, False), (65, 257, False),
        (192, 64, False), (256, 256, False)]


def _loss_setup(B, K, mixed=False):
    T, J = 3, 4
    g = torch.Generator().manual_seed(B * 31 + K)
    nb = 2 * B if mixed else B
    real = torch.rand(nb, K, generator=g)
    fake = torch.rand(nb, K, generator=g)
    names = ("h_fake", "m_real", "h_real_p", "m_fake", "h_fake_p", "m_real_p") if mixed else ("h_fake", "h_real", "m_real", "m_fake")
    f = {k: torch.rand(B, T, J, generator=g) for k in names}
    return T, J, real, fake, f


def _run_loss(L, kind, B, K, fused, offset=0):
    mixed = kind == "mixed"
    T, J, real, fake, f = _loss_setup(B, K, mixed)
    sc, eps, L_, Lmin = 4.0 / K, 0.8, 40, 10
    nprob = 4 if mixed else 3
    if fused:
        assert L.lib.kccot_sinkhorn_fused_eligible(B, L_) == 1
    sym, wsq = {"one": ("kccot_sinkhorn_loss", "kccot_sinkhorn_loss_workspace_bytes"),
                "bicausal": ("kccot_bicausal_sinkhorn_loss", "kccot_bicausal_sinkhorn_loss_workspace_bytes"),
                "mixed": ("kccot_mixed_sinkhorn_loss", "kccot_mixed_sinkhorn_loss_workspace_bytes")}[kind]
    fsym, bsym = {"bicausal": ("kccot_bicausal_sinkhorn_loss_fwd_f32", "kccot_bicausal_sinkhorn_loss_bwd_f32"),
                  "mixed": ("kccot_mixed_sinkhorn_loss_fwd_f32", "kccot_mixed_sinkhorn_loss_bwd_f32")}.get(kind, (None, None))
    ws = ws_query(L, wsq, B, K)
    R, Fv = ("R", "F") if mixed else ("real", "fake")
    ins = {R: real.to(DEV), Fv: fake.to(DEV), **{k: v.to(DEV) for k, v in f.items()}}
    feats = ["@" + k for k in f]
    Cn = "Cmix" if mixed else "C3"
    dCn = "dCmix_unit" if mixed else "dC3_unit"
    H = max(L_, 1)
    outs = {Cn: ((nprob, B, B), F32), "cost%d_out" % nprob: ((nprob,), F32), "nits_out": ((2 * nprob,), I32),
            "loss_out": ((1,), F32), "ticket": ((1,), I32)}
    head = ["@" + R, "@" + Fv, B, K, sc] + feats + [T, J, eps, L_, Lmin, THRESH, 0, "@" + Cn]
    tail = ["@cost%d_out" % nprob, "@nits_out", "@loss_out", "@ticket", "@ws", "@ws_bytes", None]
    if kind == "one" and fused:
        fsym = "kccot_sinkhorn_loss_fused_fwd_f32"
        spec = head + ["@" + dCn] + tail
        outs[dCn] = ((nprob, B, B), F32)
        regions = None
    elif kind == "one":
        fsym = "kccot_sinkhorn_loss_fwd_f32"
        spec = head + ["@u_hist", "@v_hist"] + tail
        outs.update(u_hist=((nprob, H, B), F32), v_hist=((nprob, H, B), F32))
        regions = lambda r: hist_regions(nprob, L_, B, r["nits_out"])
    else:
        if fused:
            spec = head + [None, None, "@" + dCn] + tail
            outs[dCn] = ((nprob, B, B), F32)
            regions = None
        else:
            spec = head + ["@u_hist", "@v_hist", None] + tail
            outs.update(u_hist=((nprob, H, B), F32), v_hist=((nprob, H, B), F32))
            regions = lambda r: hist_regions(nprob, L_, B, r["nits_out"])
    fwd = guarded_call(L, fsym, spec, ins, outs, ws, offset=offset, regions=regions, zero_in=("ticket",))
    gl = torch.tensor([-0.7])
    gouts = {("dF" if mixed else "dfake"): ((2 * B if mixed else B, K), F32), **{"d" + k: ((B, T, J), F32) for k in f}}
    gspec = ["@" + k for k in gouts]
    bins = dict(ins, gloss=gl.to(DEV))
    mid = ["@gloss", "@" + R, "@" + Fv, B, K, sc] + feats + [T, J]
    if kind == "one" and fused:
        bsym = "kccot_sinkhorn_loss_fused_bwd_f32"
        bins[dCn] = fwd[dCn]
        bspec = ["@gloss", "@" + dCn, "@" + R, "@" + Fv, B, K, sc] + feats + [T, J] + gspec + ["@ws", "@ws_bytes", None]
    elif kind == "one":
        bsym = "kccot_sinkhorn_loss_bwd_f32"
        bins.update({Cn: fwd[Cn], "u_hist": fwd["u_hist"], "v_hist": fwd["v_hist"], "nits": fwd["nits_out"]})
        bspec = mid + [eps, L_, "@" + Cn, "@u_hist", "@v_hist", "@nits"] + gspec + ["@ws", "@ws_bytes", None]
    else:
        if fused:
            bins[dCn] = fwd[dCn]
            bspec = mid + [eps, L_, None, None, None, None, "@" + dCn] + gspec + ["@ws", "@ws_bytes", None]
        else:
            bins.update({Cn: fwd[Cn], "u_hist": fwd["u_hist"], "v_hist": fwd["v_hist"], "nits": fwd["nits_out"]})
            bspec = mid + [eps, L_, "@" + Cn, "@u_hist", "@v_hist", "@nits", None] + gspec + ["@ws", "@ws_bytes", None]
    # (the backward's workspace is poisoned afresh: it must not depend on what the forward left there)
    bwd = guarded_call(L, bsym, bspec, bins, gouts, ws, offset=offset)
    nits = fwd["nits_out"].cpu()
    loss, Cs, grads = loss_oracle("mixed" if mixed else kind, real, fake, f, sc, eps, nits, float(gl[0]))
    for p in range(nprob):
        close(fwd[Cn][p], Cs[p], 1e-5, "%s[%d]" % (Cn, p))
    assert abs(float(fwd["loss_out"][0]) - loss) <= 1e-4 * max(abs(loss), float(fwd["cost%d_out" % nprob].abs().max())), \
        (float(fwd["loss_out"][0]), loss)
    for k in gouts:
        close(bwd[k], grads[k], GRAD_TOL, k)


@pytest.mark.parametrize("B,K,fused", LOSS)
def test_sinkhorn_loss(L, B, K, fused):
    _run_loss(L, "one", B, K, fused)


@pytest.mark.parametrize("B,K,fused", [(8, 260, True), (64, 512, False)])
def test_sinkhorn_loss_at_a_4_byte_offset(L, B, K, fused):
    _run_loss(L, "one", B, K, fused, offset=4)


@pytest.mark.parametrize("kind", ["mixed", "bicausal"])
@pytest.mark.parametrize("B,K,fused", LOSS)
def test_two_sample_losses(L, kind, B, K, fused):
    _run_loss(L, kind, B, K, fused)


# ---------------------------------------------------------------- martingale, model cells, MMD
@pytest.mark.parametrize("B,T,J", [(1, 5, 2), (7, 5, 3), (64, 30, 8), (65, 9, 17)])
def test_martingale(L, B, T, J):
    lam, sc = 1.5, 0.3
    M = torch.rand(B, T, J, generator=torch.Generator().manual_seed(B + T))
    pm = guarded_call(L, "kccot_martingale_fwd_f32", ["@M", B, T, J, lam, sc, "@pm_out", None], {"M": M.to(DEV)},
                      {"pm_out": ((1,), F32)})["pm_out"]
    Md = M.double().requires_grad_(True)
    ref = ot.scale_invariante_martingale_regularization(Md, lam, sc)
    assert abs(float(pm[0]) - float(ref)) <= 1e-5 * abs(float(ref))
    (ref * 2.5).backward()
    dM = guarded_call(L, "kccot_martingale_bwd_f32", ["@M", B, T, J, lam, sc, "@gpm", "@dM", None],
                      {"M": M.to(DEV), "gpm": torch.tensor([2.5], device=DEV)}, {"dM": ((B, T, J), F32)})["dM"]
    close(dM, Md.grad, GRAD_TOL, "dM")


def _cell64(gx, gh, c0):
    g = gx + gh
    F = c0.shape[1]
    hs = lambda v: (0.2 * v + 0.5).clamp(0, 1)
    i, f, cc, o_ = hs(g[:, :F]), hs(g[:, F:2 * F]), torch.tanh(g[:, 2 * F:3 * F]), hs(g[:, 3 * F:])
    c = f * c0 + i * cc
    return c, o_ * torch.tanh(c)


@pytest.mark.parametrize("B,F,HW,offset", [(1, 1, 1, 0), (3, 5, 7, 0), (2, 8, 16, 0), (1, 3, 33, 0), (2, 8, 16, 4)])
def test_convlstm_cell(L, B, F, HW, offset):
    g = torch.Generator().manual_seed(B * 100 + F * 10 + HW)
    gx, gh = 4 * torch.randn(B, 4 * F, HW, generator=g), 2 * torch.randn(B, 4 * F, HW, generator=g)
    c0 = torch.randn(B, F, HW, generator=g)
    ins = {"gx": gx.to(DEV), "gh": gh.to(DEV), "c_prev": c0.to(DEV)}
    fwd = guarded_call(L, "kccot_convlstm_cell_fwd_f32", ["@gx", "@gh", "@c_prev", B, F, HW, "@c_out", "@h_out", None], ins,
                       {"c_out": ((B, F, HW), F32), "h_out": ((B, F, HW), F32)}, offset=offset)
    a = [t.double().requires_grad_(True) for t in (gx, gh, c0)]
    c1, h1 = _cell64(*a)
    close(fwd["c_out"], c1, 0, "c", atol=2e-6)
    close(fwd["h_out"], h1, 0, "h", atol=2e-6)
    dh, dc = torch.randn(B, F, HW, generator=g), torch.randn(B, F, HW, generator=g)
    bwd = guarded_call(L, "kccot_convlstm_cell_bwd_f32", ["@gx", "@gh", "@c_prev", "@c_out", "@dh", "@dc_out", B, F, HW, "@dg",
                                                          "@dc_prev", None],
                       dict(ins, c_out=fwd["c_out"], dh=dh.to(DEV), dc_out=dc.to(DEV)),
                       {"dg": ((B, 4 * F, HW), F32), "dc_prev": ((B, F, HW), F32)}, offset=offset)
    ((c1 * dc.double()).sum() + (h1 * dh.double()).sum()).backward()
    for got, ref, k in ((bwd["dg"], a[0].grad, "dg"), (bwd["dc_prev"], a[2].grad, "dc_prev")):
        close(got, ref, 0, k, atol=3e-6 * max(1.0, float(ref.abs().max())))


@pytest.mark.parametrize("N,C,HW", [(1, 3, 33), (3, 5, 7), (6, 32, 64), (2, 256, 16), (7, 1, 1)])
def test_channel_layernorm(L, N, C, HW):
    g = torch.Generator().manual_seed(N + C + HW)
    x = 2 * torch.randn(N, C, HW, generator=g) + 0.7
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    eps = 1e-3
    fwd = guarded_call(L, "kccot_channel_layernorm_fwd_f32", ["@x", "@gamma", "@beta", N, C, HW, eps, "@y", "@mean", "@rstd", None],
                       {"x": x.to(DEV), "gamma": gamma.to(DEV), "beta": beta.to(DEV)},
                       {"y": ((N, C, HW), F32), "mean": ((N, HW), F32), "rstd": ((N, HW), F32)})
    xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu = xd.mean(1, keepdim=True)
    var = ((xd - mu) ** 2).mean(1, keepdim=True)
    y = (xd - mu) / torch.sqrt(var + eps) * gd[None, :, None] + bd[None, :, None]
    close(fwd["y"], y, 0, "y", atol=5e-6 * float(y.abs().max()))
    dy = torch.randn(N, C, HW, generator=g)
    nch = int(L.lib.kccot_channel_layernorm_chunks(N, C, HW))
    bwd = guarded_call(L, "kccot_channel_layernorm_bwd_f32", ["@dy", "@x", "@gamma", "@mean", "@rstd", N, C, HW, "@dx", "@partials",
                                                              None],
                       {"dy": dy.to(DEV), "x": x.to(DEV), "gamma": gamma.to(DEV), "mean": fwd["mean"], "rstd": fwd["rstd"]},
                       {"dx": ((N, C, HW), F32), "partials": ((nch, 2, C), F32)})
    (y * dy.double()).sum().backward()
    tol = lambda r: 2e-5 * max(1.0, float(r.abs().max()))
    close(bwd["dx"], xd.grad, 0, "dx", atol=tol(xd.grad))
    p = bwd["partials"].double().sum(0)
    close(p[0], gd.grad, 0, "dgamma", atol=tol(gd.grad))
    close(p[1], bd.grad, 0, "dbeta", atol=tol(bd.grad))


@pytest.mark.parametrize("B,gamma", [(1, 0.5), (7, 0.1), (64, 0.02), (65, 0.05), (129, 0.01)])
def test_rbf_mmd(L, B, gamma):
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 9, generator=g)
    y = (x + 0.3 * torch.rand(B, 9, generator=g))
    D3 = torch.stack([((a[:, None] - b[None]) ** 2).sum(-1) for a, b in ((x, y), (x, x), (y, y))]).float()
    fwd = guarded_call(L, "kccot_rbf_mmd_f32", ["@D3", B, gamma, "@K3_out", "@mmd_out", None], {"D3": D3.to(DEV)},
                       {"K3_out": ((3, B, B), F32), "mmd_out": ((1,), F32)})
    Dd = D3.double().requires_grad_(True)
    K = torch.exp(-gamma * Dd)
    m = K[1].mean() + K[2].mean() - 2 * K[0].mean()
    close(fwd["K3_out"], K, 0, "K3", rtol=2e-5, atol=1e-7)
    assert abs(float(fwd["mmd_out"][0]) - float(m)) < 1e-5 * max(abs(float(m)), 1e-3)
    (m * 3.0).backward()
    gD = guarded_call(L, "kccot_rbf_mmd_bwd_f32", ["@K3", B, gamma, "@gmmd", "@gD3", None],
                      {"K3": fwd["K3_out"], "gmmd": torch.tensor([3.0], device=DEV)}, {"gD3": ((3, B, B), F32)})["gD3"]
    close(gD, Dd.grad, 2e-5, "gD3")


# ---------------------------------------------------------------- kernel smoothing
# (the three shapes where the fused 3-D adjoint's grid outgrew the workspace's tie records come first)
SMOOTH = [((1, 16, 8, 64, 1), 3, dict(smooth_fused3=2, smooth_bwd_fold=2)),
          ((1, 30, 8, 64, 1), 3, dict(smooth_fused3=2, smooth_bwd_fold=2)),
          ((8192, 8, 8, 8, 1), 3, {}),
          ((70, 9, 8, 8, 1), 3, dict(smooth_fused3=2, smooth_bwd_fold=2)),     # 70 tiles against 74 records: the fused adjoint fits
          ((2, 5, 8, 5, 3), 3, {}), ((2, 5, 8, 5, 3), 3, dict(smooth_fused3=2, smooth_bwd_fold=2)),
          ((1, 6, 10, 7, 1), 4, {}), ((2, 6, 10, 8, 3), 4, dict(smooth_fused3=2)),
          ((3, 9, 8, 12, 1), 3, dict(smooth_fused3=0, smooth_bwd_fold=0)), ((2, 9, 8, 12, 3), 3, dict(smooth_stream=0)),
          ((2, 10, 9, 16, 1), 3, dict(smooth_generic=1)), ((2, 12, 8, 16, 3), 3, dict(smooth_fused3=1, smooth_bwd_fold=2)),
          ((1, 17, 8, 32, 1), 3, dict(smooth_fused3=2, smooth_bwd_fold=0))]


@pytest.mark.parametrize("shape,R,opts", SMOOTH)
def test_smoothing(L, shape, R, opts, offset=0):
    from oracle import smoothing_torch as st
    B, H, T, W, C = shape
    sigma = 2.1
    ws = ws_query(L, "kccot_smooth_workspace_bytes", B, H, T, W, C)
    g = torch.Generator().manual_seed(sum(shape) + R)
    v = torch.rand(shape, generator=g)
    gout = torch.randn(shape, generator=g)
    big = v.numel() > 1 << 20
    for axes, dims in (((L.SMOOTH_T | L.SMOOTH_H | L.SMOOTH_W), (2, 1, 3)), (L.SMOOTH_T, (2,))):
        if big and dims == (2,):
            continue
        with L.options(**opts):
            fwd = guarded_call(L, "kccot_smooth_fwd_f32", ["@in", B, H, T, W, C, sigma, R, axes, "@out", "@max_inout", "@ws",
                                                           "@ws_bytes", None], {"in": v.to(DEV)},
                               {"out": (shape, F32), "max_inout": ((1,), F32)}, ws, offset=offset)
            bins = {"gout": gout.to(DEV), "out": fwd["out"], "max_in": fwd["max_inout"]}
            bwd = guarded_call(L, "kccot_smooth_bwd_f32", ["@gout", "@out", "@max_in", B, H, T, W, C, sigma, R, axes, "@din", "@ws",
                                                           "@ws_bytes", None], bins, {"din": (shape, F32)}, ws, offset=offset)
            if not big:
                stats = guarded_call(L, "kccot_smooth_bwd_sharded_f32",
                                     ["@gout", "@out", "@max_in", "@stats_inout", B, H, T, W, C, sigma, R, axes | L.SMOOTH_STATS_ONLY,
                                      "@din", "@ws", "@ws_bytes", None], bins, {"stats_inout": ((2,), F32), "din": (shape, F32)},
                                     ws, offset=offset, regions=lambda r: {"din": torch.zeros(shape, dtype=torch.bool)})
                ext = guarded_call(L, "kccot_smooth_bwd_sharded_f32",
                                   ["@gout", "@out", "@max_in", "@stats", B, H, T, W, C, sigma, R, axes | L.SMOOTH_EXTERNAL_STATS,
                                    "@din", "@ws", "@ws_bytes", None], dict(bins, stats=stats["stats_inout"]), {"din": (shape, F32)},
                                   ws, offset=offset)
        vd = v.double().requires_grad_(True)
        s = st.smooth(vd, sigma, R, dims)
        close(fwd["out"], s, 0, "out", rtol=1e-5, atol=1e-6)
        assert float(fwd["out"].max()) == 1.0
        (s * gout.double()).sum().backward()
        tol = 2e-4 * float(vd.grad.abs().max())
        close(bwd["din"], vd.grad, 0, "din", atol=tol)
        if not big:
            close(ext["din"], vd.grad, 0, "din (sharded)", atol=tol)
            o64, g64 = fwd["out"].double(), gout.double().to(DEV)
            assert abs(float(stats["stats_inout"][0]) - float((o64 * g64).sum())) <= 1e-5 * float((o64 * g64).abs().sum())
            assert float(stats["stats_inout"][1]) == float((fwd["out"] == 1).sum())


@pytest.mark.parametrize("shape,R,opts", [((2, 5, 8, 5, 3), 3, {}), ((1, 16, 8, 64, 1), 3, dict(smooth_fused3=2, smooth_bwd_fold=2)),
                                          ((2, 12, 8, 16, 3), 3, dict(smooth_fused3=2)), ((1, 6, 10, 7, 1), 4, {})])
def test_smoothing_at_a_4_byte_offset(L, shape, R, opts):
    test_smoothing(L, shape, R, opts, offset=4)


# ---------------------------------------------------------------- the canary debug aid, in a child process
_CANARY_CHILD = r"""
import torch
from kccotgan_amd import gan_utils as G, _lib
from kccotgan_amd.data_utils import KernelSmoothing
assert _lib._CANARY
d = "cuda"
g = torch.Generator(device=d).manual_seed(0)
B, T, H, W, J = 8, 6, 4, 8, 3
r = lambda *s: torch.rand(*s, device=d, generator=g)
real, fake = r(B, H, T, W, 1), r(B, H, T, W, 1).requires_grad_(True)
f = {k: r(B, T, J).requires_grad_(True) for k in ("h_fake", "m_real", "h_real", "m_fake", "h_real_p", "h_fake_p", "m_real_p")}
loss = G.compute_sinkhorn_loss(real, fake, 0.01, 0.8, 30, f["h_fake"], f["m_real"], f["h_real"], f["m_fake"], video=True)
loss.backward()
loss = G.compute_mixed_sinkhorn_loss(real, fake, r(B, H, T, W, 1), r(B, H, T, W, 1), 0.01, 0.8, 30, f["h_fake"], f["m_real"],
                                     f["h_real_p"], f["m_fake"], f["h_fake_p"], f["m_real_p"], video=True)
loss.backward()
loss = G.compute_bicausal_sinkhorn_loss(real, fake, 0.01, 0.8, 30, f["h_fake"], f["m_real"], f["h_real"], f["m_fake"], video=True)
loss.backward()
ks = KernelSmoothing(6, 6)
v = r(2, 9, 8, 12, 1).requires_grad_(True)
(ks.gaussian_convolution3D(v, 2.0) * r(2, 9, 8, 12, 1)).sum().backward()
(ks.temporal_convolution(v, 2.0) * r(2, 9, 8, 12, 1)).sum().backward()
G.scale_invariante_martingale_regularization(f["m_real"], 1.5, 0.3).backward()
torch.cuda.synchronize()
_lib._verify_guards("end")
print("canary child ok")
"""


def test_canary_mode_runs_the_public_api_clean():
    """KCCOT_DEBUG_CANARY=1 (guard zones around every buffer the wrappers hand to the library, checked after every call):
    one forward and backward of each loss, both smoothings and the martingale penalty in a fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, KCCOT_DEBUG_CANARY="1")
    p = subprocess.run([sys.executable, "-c", _CANARY_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "canary child ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])
