"""CPU-side checks of the L1 ground cost (KCCOT_COST_L1 of include/kccot.h, its adjoint in include/kccot_l1.h; not reference
behaviour): the oracle of the GPU tests (tests/l1_oracle.py) against autograd on inputs full of ties, a plain float32 evaluation
of the definition against the caps the GPU tests may not exceed, the header against the ctypes table and as strict C99, the
argument rules that are decided before any launch (pointers that are never dereferenced), every refused flag combination, and
the Python path's refusals."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import l1_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kccot_l1_cost3_bwd_f32", "kccot_l1_cost3_bwd_workspace_bytes", "kccot_l1_cost_bwd_f32", "kccot_l1_cost_bwd_workspace_bytes"]
SC = lo.f32(1.0 / 15.0)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bx,By,K", [(3, 5, 7), (9, 4, 40), (8, 8, 64)])
def test_closed_form_adjoints_equal_autograd_on_ties(Bx, By, K):
    x, y = (v.double() for v in lo.rows("ties", Bx, By, K, 3))
    assert int((x[:, None, :] == y[None, :, :]).sum()) > Bx * By * K // 20, "the inputs tie often"
    g = lo.upstream((Bx, By), 4).double()
    xv, yv = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    (lo.l1_block(xv, yv, SC) * g).sum().backward()
    for got, ref in ((lo.adjoint_x(g, x, y, SC), xv.grad), (lo.adjoint_y(g, x, y, SC), yv.grad)):
        assert float((got - ref).abs().max()) <= 1e-12
    # x == y: the tensor receives both contributions; the diagonal ties everywhere
    gs = lo.upstream((Bx, Bx), 5).double()
    xs = x.clone().requires_grad_(True)
    Cs = lo.l1_block(xs, xs, SC)
    assert float(Cs.detach().diagonal().abs().max()) == 0.0 and torch.equal(Cs.detach(), Cs.detach().t())
    (Cs * gs).sum().backward()
    assert float((lo.adjoint_same(gs, x, SC) - xs.grad).abs().max()) <= 1e-12


@pytest.mark.parametrize("B", [2, 8])
def test_loss_form_adjoint_equals_autograd_and_the_context_ties_give_exact_zeros(B):
    real, fake = (v.double().reshape(B, -1) for v in lo.videos("ties", B, 6))
    g3 = lo.upstream((3, B, B), 7).double()
    fv = fake.clone().requires_grad_(True)
    C3 = torch.stack((lo.l1_block(real, fv, SC), lo.l1_block(real, real, SC), lo.l1_block(fv, fv, SC)))
    (C3 * g3).sum().backward()
    d = lo.adjoint_fake(g3, real, fake, SC)
    assert float((d - fv.grad).abs().max()) <= 1e-12
    # sgn(0) = 0: with the xy term alone, at i = j, every context position contributes exactly 0
    only = torch.zeros_like(g3)
    only[0] = torch.diag(g3[0].diagonal())
    ctx = lo.context_mask(B)
    assert torch.equal(fake[ctx], real[ctx])
    assert float(lo.adjoint_fake(only, real, fake, SC)[ctx].abs().max()) == 0.0


@pytest.mark.parametrize("Bx,By,K,offset", lo.FWD_SHAPES)
@pytest.mark.parametrize("kind", ["noise", "ties"])
def test_float32_evaluation_in_the_kernels_chunk_shape_stays_inside_the_caps(Bx, By, K, offset, kind):
    x, y = lo.rows(kind, Bx, By, K, 11)
    ref = lo.l1_block(x.double(), y.double(), SC)
    got = lo.fp32_forward_like_the_kernel(x, y, SC, lo.fwd_chunk(K)).double()
    nz = ref > 0
    err = float(((got - ref).abs()[nz] / ref[nz]).max()) if bool(nz.any()) else 0.0
    print("%s (%d,%d,%d): float32 forward |C - ref| / ref %.3e (cap %.3e)" % (kind, Bx, By, K, err, lo.CAP_FWD))
    assert err <= lo.CAP_FWD and torch.equal(got[~nz], ref[~nz])
    # the adjoint in float32, summed sequentially over the sources, against its cap
    g = lo.upstream((Bx, By), 12)
    ref_d = lo.adjoint_x(g.double(), x.double(), y.double(), SC)
    acc = torch.zeros((Bx, K), dtype=torch.float32)
    for c in range(By):
        acc = acc + g[:, c:c + 1] * torch.sign(x - y[c:c + 1])
    got_d = (acc * torch.tensor(SC, dtype=torch.float32)).double()
    if float(ref_d.abs().max()) > 0:
        e = float((got_d - ref_d).abs().max()) / float(ref_d.abs().max())
        cap = lo.bwd_cap("x", g, ref_d, SC)
        print("%s (%d,%d,%d): float32 adjoint |d - ref| / max|ref| %.3e (cap %.3e)" % (kind, Bx, By, K, e, cap))
        assert e <= cap


# ---- the header ----------------------------------------------------------------------------------------------------------------
def _decls(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(2), (m.group(1), m.group(3)))
                for m in re.finditer(r"\b(int|size_t)\s+(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_and_ctypes_table_agree_and_stay_outside_the_versioned_surface():
    from kccotgan_amd import _lib
    decls = _decls("kccot_l1.h")
    assert sorted(decls) == NAMES and sorted(_lib.L1_SIGNATURES) == NAMES
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64,
             "unsigned": ctypes.c_uint}
    for name, (ret, args) in decls.items():
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        res, argtypes = _lib.L1_SIGNATURES[name]
        assert res is ctype[ret] and argtypes == want, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctype[ret] and list(fn.argtypes) == want
    assert not set(NAMES) & set(_decls("kccot.h")) and not set(NAMES) & set(_lib.SIGNATURES)
    assert _lib.COST_L1 == 1024 and re.search(r"#define KCCOT_COST_L1 1024u", open(os.path.join(ROOT, "include", "kccot.h")).read())
    assert _lib.lib.kccot_version() == 301


def test_header_compiles_as_strict_c99(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_l1.h"\nint main(void) { return (int)KCCOT_COST_L1 - 1024; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- argument rules ------------------------------------------------------------------------------------------------------------
P = ctypes.c_void_p
G_, X_, Y_, DX_, DY_, WS_ = 1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 30      # never dereferenced


def _bwd(**kw):
    from kccotgan_amd import _lib
    a = dict(g=G_, x=X_, y=Y_, Bx=3, By=5, K=7, flags=0, dx=DX_, dy=DY_, ws=WS_, wsb=1 << 20)
    a.update(kw)
    p = lambda v: None if v is None else P(v)
    return _lib.lib.kccot_l1_cost_bwd_f32(p(a["g"]), p(a["x"]), p(a["y"]), a["Bx"], a["By"], a["K"], SC, a["flags"], p(a["dx"]),
                                          p(a["dy"]), p(a["ws"]), a["wsb"], None)


def _bwd3(**kw):
    from kccotgan_amd import _lib
    a = dict(g=G_, real=X_, fake=Y_, B=4, K=7, d=DX_, ws=WS_, wsb=1 << 20)
    a.update(kw)
    p = lambda v: None if v is None else P(v)
    return _lib.lib.kccot_l1_cost3_bwd_f32(p(a["g"]), p(a["real"]), p(a["fake"]), a["B"], a["K"], SC, p(a["d"]), p(a["ws"]),
                                           a["wsb"], None)


def test_adjoint_argument_rules_return_their_codes_before_any_launch():
    from kccotgan_amd import _lib
    err = _lib.lib.kccot_last_error
    for kw in ("g", "x", "y"):
        assert _bwd(**{kw: None}) == _lib.EINVAL and b"null" in err(), kw
    assert _bwd(dx=None, dy=None) == _lib.EINVAL and b"null output" in err()
    for kw in ("Bx", "By", "K"):
        for bad in (0, -2):
            assert _bwd(**{kw: bad}) == _lib.EINVAL and b"shape" in err(), (kw, bad)
    for flags in (2, 4, 1024, 1 | 2, 1 << 31):
        assert _bwd(flags=flags, dy=None) == _lib.EINVAL and b"flags" in err(), flags
    # SAME: x is y, square, no dy
    assert _bwd(flags=1) == _lib.EINVAL and b"SAME" in err()
    assert _bwd(flags=1, y=X_, By=3) == _lib.EINVAL and b"SAME" in err()                  # dy given
    assert _bwd(flags=1, y=X_, dy=None) == _lib.EINVAL and b"SAME" in err()               # Bx != By
    # an output overlapping an input or the other output (g 60 bytes, x 84, y 140)
    for kw in (dict(dx=G_), dict(dx=G_ + 56), dict(dx=X_ + 80), dict(dx=Y_ - 80), dict(dy=G_ - 136), dict(dy=X_), dict(dy=Y_ + 4),
               dict(dy=DX_ + 80), dict(dx=DY_ + 136)):
        assert _bwd(**kw) == _lib.EINVAL and b"alias" in err(), kw
    # just clear of each other, a workspace one byte short: as far as the workspace check
    need = _lib.lib.kccot_l1_cost_bwd_workspace_bytes(3, 5)
    assert need > 0 and need % 4 == 0
    assert _bwd(dx=X_ + 84, wsb=need - 1) == _lib.EWORKSPACE and b"workspace" in err()
    assert _bwd(ws=None) == _lib.EWORKSPACE
    assert _bwd(dy=None, wsb=need - 1) == _lib.EWORKSPACE and _bwd(dx=None, wsb=0) == _lib.EWORKSPACE
    assert _bwd(flags=1, y=X_, By=3, dy=None, wsb=0) == _lib.EWORKSPACE
    # too large to index
    assert _bwd(Bx=65535 * 8 + 1, dy=None, dx=1 << 60) == _lib.EUNSUPPORTED
    assert _bwd(K=1 << 50, dx=1 << 61, dy=None) == _lib.EUNSUPPORTED
    # the loss form
    for kw in ("g", "real", "fake", "d"):
        assert _bwd3(**{kw: None}) == _lib.EINVAL and b"null" in err(), kw
    for kw in ("B", "K"):
        for bad in (0, -1):
            assert _bwd3(**{kw: bad}) == _lib.EINVAL and b"shape" in err(), (kw, bad)
    for d in (G_, G_ + 188, X_ + 4, Y_ - 108, Y_ + 108):        # g3 192 bytes, the videos 112
        assert _bwd3(d=d) == _lib.EINVAL and b"alias" in err(), d
    need3 = _lib.lib.kccot_l1_cost3_bwd_workspace_bytes(4)
    assert _bwd3(d=Y_ + 112, wsb=need3 - 1) == _lib.EWORKSPACE and _bwd3(ws=None) == _lib.EWORKSPACE
    assert _bwd3(B=65535 * 8 + 1, d=1 << 60) == _lib.EUNSUPPORTED


def test_workspace_queries_hold_the_coefficient_matrices_only():
    from kccotgan_amd import _lib
    q, q3 = _lib.lib.kccot_l1_cost_bwd_workspace_bytes, _lib.lib.kccot_l1_cost3_bwd_workspace_bytes
    assert q(0, 4) == q(4, 0) == q(-1, 4) == q3(0) == q3(-5) == 0
    for Bx, By in ((1, 1), (3, 5), (64, 64), (65, 130), (512, 512)):
        pad = lambda n: (n + 7) // 8 * 8
        up = lambda b: (b + 255) // 256 * 256
        assert q(Bx, By) == up(By * pad(Bx) * 4) + up(Bx * pad(By) * 4)
    assert q3(64) == 2 * 64 * 64 * 4 and q3(70) == (2 * 70 * 72 * 4 + 255) // 256 * 256


def test_every_refused_flag_combination_returns_einval_with_a_reason():
    from kccotgan_amd import _lib
    lib, err, L1 = _lib.lib, _lib.lib.kccot_last_error, _lib.COST_L1
    a, b, c, w = P(X_), P(Y_), P(DX_), P(WS_)
    f4 = (a, b, c, a)                                       # features (never read)

    def cost(flags, x=a, y=b):
        return lib.kccot_pairwise_cost_f32(x, y, 4, 4, 8, SC, a, b, None, None, 3, 2, flags, c, w, 1 << 30, None)

    def cost3(flags):
        return lib.kccot_pairwise_cost3_f32(a, b, 4, 8, SC, *f4, 3, 2, flags, c, w, 1 << 30, None)

    refused = dict(FORCE_MFMA=_lib.COST_FORCE_MFMA, PARTIAL_ONLY=_lib.COST_PARTIAL_ONLY, GRAM_SUMS_ONLY=_lib.COST_GRAM_SUMS_ONLY,
                   FROM_GRAM_SUMS=_lib.COST_FROM_GRAM_SUMS, BICAUSAL_TERM_ONLY=_lib.COST_BICAUSAL_TERM_ONLY,
                   CAUSAL_ADD=_lib.COST_CAUSAL_ADD, RBF_SUM=_lib.COST_RBF_SUM, CMIX_GIVEN=_lib.MIXED_CMIX_GIVEN)
    for name, bit in refused.items():
        for fn in (cost, cost3):
            assert fn(L1 | bit) == _lib.EINVAL and len(err()) > 20, (name, fn.__name__)
    for name in ("FORCE_MFMA", "PARTIAL_ONLY", "GRAM_SUMS_ONLY", "FROM_GRAM_SUMS"):
        assert cost3(L1 | refused[name]) == _lib.EINVAL and b"KCCOT_COST_L1" in err(), name
        assert cost(L1 | refused[name]) == _lib.EINVAL and b"KCCOT_COST_L1" in err(), name
    # what combines gets as far as the workspace check (no device is touched)
    for flags, kw in ((L1, {}), (L1 | _lib.COST_FORCE_DIRECT, {}), (L1 | _lib.COST_SAME, dict(y=a)),
                      (L1 | _lib.COST_SAME | _lib.COST_FORCE_DIRECT, dict(y=a))):
        assert lib.kccot_pairwise_cost_f32(a, kw.get("y", b), 4, 4, 8, SC, a, b, None, None, 3, 2, flags, c, None, 0, None) == \
            _lib.EWORKSPACE, flags
    assert lib.kccot_pairwise_cost3_f32(a, b, 4, 8, SC, *f4, 3, 2, L1 | _lib.COST_FORCE_DIRECT, c, None, 0, None) == _lib.EWORKSPACE
    assert cost(L1 | _lib.COST_SAME) == _lib.EINVAL and b"SAME" in err()              # SAME keeps its own rule: x is y
    # the other entry points that take cost flags refuse it
    assert lib.kccot_pairwise_cost_bwd_f32(a, a, b, 4, 4, 8, SC, a, b, 3, 2, L1, None, None, c, None, None, 0, None) == _lib.EINVAL
    assert b"KCCOT_COST_L1" in err()
    i4 = (a, b, 4, 8, SC, *f4, 3, 2, 1.0, 100, 100, 0.01)
    big = 1 << 40
    calls = {
        "sinkhorn_loss_fwd": lambda fl: lib.kccot_sinkhorn_loss_fwd_f32(*i4, fl, c, c, c, c, c, c, c, w, big, None),
        "sinkhorn_loss_fused_fwd": lambda fl: lib.kccot_sinkhorn_loss_fused_fwd_f32(*i4, fl, c, c, c, c, c, c, w, big, None),
        "bicausal_sinkhorn_loss_fwd": lambda fl: lib.kccot_bicausal_sinkhorn_loss_fwd_f32(*i4, fl, c, c, c, None, c, c, c, c, w, big, None),
        "weighted_sinkhorn_loss_fwd": lambda fl: lib.kccot_weighted_sinkhorn_loss_fwd_f32(*i4, fl, a, b, c, c, c, c, c, c, c, w, big, None),
        "conditional_sinkhorn_loss_fwd": lambda fl: lib.kccot_conditional_sinkhorn_loss_fwd_f32(*i4, fl, a, None, 1, c, c, c, c, c, c, w, big, None),
        "mixed_sinkhorn_loss_fwd": lambda fl: lib.kccot_mixed_sinkhorn_loss_fwd_f32(a, b, 4, 8, SC, a, b, a, b, a, b, 3, 2, 1.0, 100, 100,
                                                                                 0.01, fl, c, c, c, None, c, c, c, c, w, big, None),
    }
    for name, f in calls.items():
        for fl in (L1, L1 | _lib.COST_FORCE_DIRECT):
            assert f(fl) == _lib.EINVAL, (name, fl)
            assert b"L1" in err(), (name, err())


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_ground_cost_keyword_is_keyword_only_defaults_to_l2_and_refuses_other_values():
    from kccotgan_amd import gan_utils as G
    for fn in (G.cost_xy, G.modified_cost, G.bi_causal_modified_cost, G.benchmark_sinkhorn, G.compute_sinkhorn,
               G.compute_sinkhorn_loss):
        p = inspect.signature(fn).parameters["ground_cost"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "l2", fn.__name__
    for fn in (G.compute_mixed_sinkhorn_loss, G.compute_weighted_sinkhorn_loss, G.compute_conditional_sinkhorn_loss,
               G.compute_kernel_conditional_sinkhorn_loss, G.compute_weighted_sinkhorn):
        assert "ground_cost" not in inspect.signature(fn).parameters, fn.__name__
    # the bi-causal loss keeps the parameter list of compute_sinkhorn_loss (tests/test_bicausal_oracle.py), but has no L1 form
    v, f = torch.zeros((2, 2, 3, 2, 1)), torch.zeros((2, 3, 1))
    with pytest.raises(NotImplementedError, match="L1"):
        G.compute_bicausal_sinkhorn_loss(v, v, SC, 0.8, 100, f, f, f, f, ground_cost="l1")
    with pytest.raises(ValueError, match="ground_cost"):
        G.compute_bicausal_sinkhorn_loss(v, v, SC, 0.8, 100, f, f, f, f, ground_cost="nope")
    x, y = lo.rows("noise", 3, 3, 8, 1)
    x, y = x.view(3, 2, 4), y.view(3, 2, 4)
    h = torch.zeros((3, 2, 1))
    for bad in ("nope", "L1", None, 1):
        for call in (lambda: G.cost_xy(x, y, SC, ground_cost=bad), lambda: G.modified_cost(x, y, h, h, SC, ground_cost=bad),
                     lambda: G.bi_causal_modified_cost(x, y, h, h, h, h, SC, ground_cost=bad),
                     lambda: G.benchmark_sinkhorn(x, y, SC, ground_cost=bad),
                     lambda: G.compute_sinkhorn(x, y, h, h, SC, ground_cost=bad),
                     lambda: G.compute_sinkhorn_loss(x, y, SC, 0.8, 100, h, h, h, h, video=False, ground_cost=bad)):
            with pytest.raises(ValueError, match="ground_cost"):
                call()
    # no CPU path for either cost
    from kccotgan_amd import _lib
    for gc in ("l1", "l2"):
        with pytest.raises(_lib.KccotError):
            G.cost_xy(x, y, SC, ground_cost=gc)


def test_trainer_refuses_the_exclusive_combinations_before_it_builds_anything():
    from kccotgan_amd.kernel_train import KCCOTTrainer
    p = inspect.signature(KCCOTTrainer.__init__).parameters["ground_cost"]
    assert p.default == "l2"
    for kw in (dict(mixed_sinkhorn=True), dict(bi_causal=True), dict(conditional_bandwidth=0.5)):
        with pytest.raises(ValueError, match="ground_cost"):
            KCCOTTrainer(2, ground_cost="l1", device="cpu", **kw)
    with pytest.raises(NotImplementedError, match="ground_cost"):
        KCCOTTrainer(2, ground_cost="l1", device="cpu", group=object())
    with pytest.raises(ValueError, match="ground_cost"):
        KCCOTTrainer(2, ground_cost="nope", device="cpu")
