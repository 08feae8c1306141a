"""The causal term sc sum_{t<T-1,q} h[i,t,q] (M[j,t+1,q] - M[j,t,q]) and its feature gradients held to float64 PAST ONE
k-CHUNK.  causal_tile16 (csrc/cost_internal.h), bicausal_cost_add (csrc/bicausal.hip) and mixed_causal_add (csrc/mixed.hip)
walk k = t J + q over KK = (T-1) J values in LDS chunks of 256; the default features (T = 30, J = 8: KK = 232) and nearly
every other test stay inside the first chunk.  Here every host of the term runs at

  (T, J)     KK    TJ    what it holds
  (30, 8)    232   240   control: one ragged chunk, as everywhere else in the suite
  (33, 8)    256   264   exactly one full chunk, no second trip
  (34, 8)    264   272   second chunk of 8 values
  (258, 1)   257   258   J = 1, second chunk of ONE value, TJ not a multiple of 16
  (2, 300)   300   600   T = 2, the M[k + J] stride longer than a chunk
  (48, 8)    376   384   configs[4]
  (65, 16)   1024  1040  four full chunks, the last one not ragged
  (1, 8)     0     8     no causal term: the output bits are those of sc 0, every feature gradient is exactly zero

through the C ABI on the guarded buffers of tests/abi_guard.py (guard words are NaNs: a clamp that reads past a feature
tensor turns up as a NaN in the result; test_gpu_abi_bounds.guarded_call checks guard zones, untouched inputs, fully written
outputs and independence of the workspace contents on every call).

Forward: the videos are ZERO (K = 256, the smallest K every Gram path accepts), so every path produces the distance part
as exactly 0 and the output is sc causal alone -- held relative to the causal term itself, not to max|C|.  Hosts (FWD):
  pair_direct, pair_direct_h2, pair_same_direct   kccot_pairwise_cost_f32, FORCE_DIRECT: cost_finalize (cost.hip), one and
                                                  two causal terms, (17, 33) and x == y at B = 33
  pair_mfma, pair_mfma_h2, pair_same_mfma         the same with FORCE_MFMA: the extra workgroups of gram_reduce (MG = 16)
  cost3_b64, cost3_b40                            kccot_pairwise_cost3_f32 on the compact record: the spare workgroups of
                                                  gram128_partial_x3ws (MG = 4; B = 40 has more than 32 rows per operand, so it
                                                  takes the compact record too: 27 ragged tiles on 16 workgroups)
  cost3_b24, cost3_b64_gram_f32                   gram_reduce's extra workgroups (B <= 32: no compact record; gram_f32 = 1)
  cost3_b64_split                                 GRAM_SUMS_ONLY then FROM_GRAM_SUMS: causal_pre_only
  cost3_b192                                      the blocked 64-row path: run_gram per 64 x 64 block, written with the
                                                  matrix's row pitch, the mirror block's own term as a second slot
  cost3_b128_tiles128, cost3_b128, cost3_b256     cost_tiled.hip (cost_tile256 = 0), the half panel and the 256-row tiles of
                                                  cost_tile256.hip
  rows_b65                                        kccot_pairwise_cost3_rows_f32, rows 3 .. 63: cost_finalize on row blocks
  rows_gram_32_128, rows_gram_64_256              kccot_pairwise_cost3_rows_gram_f32 (cost_rows.hip), row_begin 32 / 128
  bicausal_b17, bicausal_b64                      COST_BICAUSAL_TERM_ONLY on a zero C3: bicausal_cost_add
  COST_CAUSAL_ADD (mixed_causal_add)              the three shapes test_gpu_mixed_flag_bounds.py lacks, on a zero block
Expected: oracle.gan_utils_torch.causal_term in float64 on the pairings of gan_utils.py:221-223 (xy: h_fake / m_real, xx:
h_real / m_real, yy: h_fake / m_fake) and the bi-causal second pairing (h_real / m_fake).  One reference per (T, J), on 256
samples drawn once; every case reads a sub-block of it.

Backward: the same zero videos, a seeded random dC, all four feature gradients in full, dfake exactly zero.
  bwd_b64 / b40 / b8, one launch and two       the wave tasks of apply_coeffs_x3_loss3 (both B64 instantiations; K = 256
                                               makes the tasks outnumber the producer waves, gx = ceil(TJ / 16) up to 65)
                                               and coeffs_and_causal_grads (apply_one_launch = 0)
  bwd_b128, bwd_b192                           coeffs_and_causal_grads with more than one batch chunk of 64
  scaled_b64                                   kccot_pairwise_cost3_bwd_scaled_f32, gscale = -1.75
  rows_b65 (3, 60), rows_b128 (32, 64)         kccot_pairwise_cost3_bwd_rows_f32
  pair (17, 33), pair_same B = 33              kccot_pairwise_cost_bwd_f32: causal_grads
Expected: float64 autograd through causal_term contracted with dC.  Every shape of the table runs on the two B = 64 forms,
the other entry points take (34, 8), (258, 1) and (65, 16).

Two loss-level cases (bi-causal and mixed, B = 16, (34, 8), random videos at K = 260) with the oracle helpers and
tolerances of the ragged cases of test_gpu_bicausal_loss.py / test_gpu_mixed_loss.py: the two-term jobs and the four-problem
stack past one chunk.

Tolerance, per case, set against the reference: with S = the sum of the absolute values of the terms of an output element in
float64 (forward: sc sum |h| |dM|; gradients: the same with |g| inside) and gap = the largest |fp32 oracle - fp64 oracle| / S
over the elements of ALL outputs of the case (the same oracle function in float32 on the CPU), an element passes if
    |got - fp64| <= 4 max(gap, 2^-24) S
(4 = the project's GRAD_TOL_FACTOR: a correct fp32 sum in another order lands within a small multiple of the oracle's own
rounding distance; the floor is one rounding of the stored result).  No element is excluded; where S = 0 (the last time step
of dh, T = 1) the bound is 0 and the output must be exactly 0.  A dropped or misplaced chunk element is of the order of
S / KK ~ 1e-3 S, a dropped batch element of a gradient S / B.

Measured on an MI355X (each case prints `chunks <case> ... gap ... err ...`, -s; err = the largest |got - fp64| / S), kernels of
commit 9954935 (this module changes none); "of the bound" = the worst err / (4 max(gap, 2^-24)) of the family:
  family                                   gap                   largest err               of the bound
  pair_* (direct and MFMA: same figures)   1.0e-8 .. 4.0e-8      6.28e-8 at (2, 300)       0.26
  cost3_b24 / b40 / b64 (all three forms)  1.7e-8 .. 4.7e-8      7.47e-8 at (2, 300)       0.31
  cost3_b128 (both), b192, b256            2.1e-8 .. 5.9e-8      9.54e-8 at (2, 300)       0.40
  rows_b65, rows_gram_*                    1.7e-8 .. 5.8e-8      9.54e-8 at (2, 300)       0.40
  bicausal_b17 / b64                       1.5e-8 .. 5.3e-8      4.23e-8 at (2, 300)       0.18
  COST_CAUSAL_ADD (fp64 accumulator)       1.7e-8 .. 2.8e-8      1.71e-8 at (2, 300)       0.07
  bwd_b64 one / two launches, all shapes   1.0e-7 .. 1.35e-7     4.24e-7 dh_real (65, 16)  0.91
  scaled_b64                               1.2e-7 .. 1.5e-7      4.17e-7 dh_real (65, 16)  0.71
  bwd_b40, bwd_b8 (one / two launches)     1.35e-7 .. 2.1e-7     2.46e-7 dh_real (258, 1)  0.44
  bwd_b128, bwd_b192, rows_b128            8.0e-8 .. 9.5e-8      2.92e-7 dh_real (258, 1)  0.84
  rows_b65, pair, pair_same (backward)     1.35e-7 .. 1.9e-7     2.61e-7 dh_fake (65, 16)  0.48
No kernel needs more than the rule allows.  The gradients come closest: causal_grads_body and the wave tasks add each output
as ONE sequential fp32 fma chain over the batch, whose error relative to S (2e-7 .. 4e-7 at the worst of 1e4 .. 1e5 elements)
does not shrink with the batch, while the oracle's pairwise sums (gap) do -- at B >= 128 the bound is set by dh_real's gap.
(T, J) = (1, 8) gives the bits of +0 on every host and exactly zero gradients.

With each of the three chunk loops stopped after its first chunk (scratch builds, never committed) the module gives:
  causal_tile16       91 failed, 123 passed: all 90 forward cases with KK > 256 on its 18 hosts, and the bi-causal loss case
  bicausal_cost_add   11 failed, 203 passed: the 10 cases with KK > 256 of bicausal_b17 / b64, and the bi-causal loss case
  mixed_causal_add     3 failed, 211 passed: the three COST_CAUSAL_ADD cases
and every (30, 8), (33, 8) and (1, 8) control passes under all three.
"""
import functools

import pytest
import torch

import abi_guard as ag
import cases
import test_gpu_bicausal_loss as BL
import test_gpu_mixed_loss as ML
from oracle import gan_utils_torch as ot
from test_gpu_abi_bounds import guarded_call, ws_query

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SC = 1.0 / 15.0
K = 256                       # zero videos: the smallest K every Gram path accepts
TOL_FACTOR = 4.0              # GRAD_TOL_FACTOR of test_gpu_parity.py
FLOOR = 2.0 ** -24
NMASTER = 256
FEATS = ("h_fake", "h_real", "m_real", "m_fake")
PAIRS = {"xy": ("h_fake", "m_real"), "xx": ("h_real", "m_real"), "yy": ("h_fake", "m_fake"), "bxy": ("h_real", "m_fake")}
SHAPES = [(30, 8), (33, 8), (34, 8), (258, 1), (2, 300), (48, 8), (65, 16), (1, 8)]
PAST = [(34, 8), (258, 1), (65, 16)]
SHAPE_ID = lambda s: "T%dJ%d" % s


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def G():
    from kccotgan_amd import gan_utils
    return gan_utils


@pytest.fixture(autouse=True)
def _defaults(L):
    defaults = {k: L.get_option(k) for k in L.option_names()}
    yield
    for k, v in defaults.items():
        L.set_option(k, v)


# ---------------------------------------------------------------- inputs and references
@functools.lru_cache(maxsize=None)
def feats(T, J):
    """The four feature tensors of a shape, NMASTER samples, drawn once; a case uses the first rows of each."""
    g = torch.Generator().manual_seed(1000 * T + J)
    return {k: torch.rand(NMASTER, T, J, generator=g) for k in FEATS}


def dev(T, J, name, n):
    return feats(T, J)[name][:n].to(DEV)


@functools.lru_cache(maxsize=None)
def master(T, J, n):
    """tag -> (fp64 oracle, fp32 oracle, S) of the four pairings on the first n samples, [n, n] each (the oracle in column
    blocks of 32: each entry is its own sum, so the blocks only bound the [n, 32, T-1, J] intermediate)."""
    f, out = feats(T, J), {}
    for tag, (hk, mk) in PAIRS.items():
        h, M = f[hk][:n], f[mk][:n]
        c64 = torch.cat([ot.causal_term(h.double(), M[j:j + 32].double(), SC) for j in range(0, n, 32)], 1)
        c32 = torch.cat([ot.causal_term(h, M[j:j + 32], SC) for j in range(0, n, 32)], 1)
        dM = (M[:, 1:] - M[:, :-1]).double().abs().reshape(n, -1)
        out[tag] = (c64, c32, SC * (h[:, :-1].double().abs().reshape(n, -1) @ dM.t()))
    return out


def expect(T, J, tags, rows, cols):
    """(fp64, fp32, S) [len(tags), rows, cols] of the pairings `tags`: sub-blocks of the master reference."""
    m = master(T, J, 65 if max(rows.stop, cols) <= 65 else NMASTER)
    return tuple(torch.stack([m[t][q][rows, :cols] for t in tags]) for q in range(3))


def check(label, T, J, got, want, want32, S):
    check_case(label, T, J, {"": (got, want, want32, S)})


def check_case(label, T, J, parts):
    """parts: output name -> (got, fp64, fp32, S).  gap is the case's: the largest |fp32 - fp64| / S over the elements of all
    its outputs; every element of every output within 4 max(gap, 2^-24) S of its fp64 value.  Prints gap and the largest
    |err| / S of each output."""
    parts = {k: (g.detach().cpu().double(), w, w32.double(), S) for k, (g, w, w32, S) in parts.items()}
    rel = lambda d, S: float((d[S > 0] / S[S > 0]).max()) if bool((S > 0).any()) else 0.0
    gap = max(rel((w32 - w).abs(), S) for _, w, w32, S in parts.values())
    bad = []
    for k, (got, w, w32, S) in parts.items():
        assert got.shape == w.shape == S.shape, (label, k, got.shape, w.shape)
        diff = (got - w).abs()
        err = rel(diff, S)
        print("chunks %-28s T=%-3d J=%-3d KK=%-4d gap %.2e err %.2e" % ((label + " " + k).strip(), T, J, (T - 1) * J, gap, err))
        ok = diff <= TOL_FACTOR * max(gap, FLOOR) * S          # a NaN compares False
        if not bool(ok.all()):
            bad.append("%s: %d of %d elements off (%d not finite), largest |err|/S %.3g" % (
                k or "output", int((~ok).sum()), ok.numel(), int((~torch.isfinite(got)).sum()), err))
        if T == 1:
            assert bool((got == 0).all()) and not bool(S.any()), "%s %s: T = 1 has no causal term" % (label, k)
    assert not bad, "%s (T=%d, J=%d), gap %.3g: %s" % (label, T, J, gap, "; ".join(bad))


# ---------------------------------------------------------------- forward
def _zeros(*shape):
    return torch.zeros(*shape, device=DEV)


def _pair(L, T, J, Bx, By, flags, two=False, same=False):
    ins = {"x": _zeros(Bx, K), "h": dev(T, J, "h_real" if same else "h_fake", Bx), "M": dev(T, J, "m_real", By)}
    if not same:
        ins["y"] = _zeros(By, K)
    if two:
        ins.update(h2=dev(T, J, "h_real", Bx), M2=dev(T, J, "m_fake", By))
    spec = ["@x", "@x" if same else "@y", Bx, By, K, SC, "@h", "@M", "@h2" if two else None, "@M2" if two else None, T, J,
            flags | (L.COST_SAME if same else 0), "@C_out", "@ws", "@ws_bytes", None]
    got = guarded_call(L, "kccot_pairwise_cost_f32", spec, ins, {"C_out": ((Bx, By), F32)},
                       ws_query(L, "kccot_pairwise_cost_workspace_bytes", Bx, By, K))["C_out"]
    w64, w32, S = expect(T, J, ("xx",) if same else (("xy", "bxy") if two else ("xy",)), slice(0, Bx), By)
    # two terms: two fp32 values added in fp32 (the oracle's bi_causal_modified_cost adds them so)
    return got, w64.sum(0), w32.sum(0), S.sum(0)


def _cost3_ins(T, J, B):
    return {"real": _zeros(B, K), "fake": _zeros(B, K), **{k: dev(T, J, k, B) for k in FEATS}}


def _cost3(L, T, J, B, opts, split=False):
    import ctypes
    ins = _cost3_ins(T, J, B)
    ws = ws_query(L, "kccot_pairwise_cost3_workspace_bytes", B, K)
    spec = lambda flags: ["@real", "@fake", B, K, SC, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, flags, "@C3", "@ws",
                          "@ws_bytes", None]
    with L.options(**opts):
        if not split:
            got = guarded_call(L, "kccot_pairwise_cost3_f32", spec(0), ins, {"C3": ((3, B, B), F32)}, ws)["C3"]
        else:
            # GRAM_SUMS_ONLY leaves the fp64 sums in its span of the workspace; FROM_GRAM_SUMS gets that span alone
            off, nd = ctypes.c_size_t(0), ctypes.c_size_t(0)
            assert L.lib.kccot_pairwise_cost3_gram_sums_span(B, K, ctypes.byref(off), ctypes.byref(nd)) == 0 and nd.value > 0
            gw, c3 = ag.guarded(ws, "workspace", "workspace"), ag.guarded(3 * B * B * 4, "output", "C3")
            gi = {k: ag.guarded_input(k, v) for k, v in ins.items()}
            rc = L.lib.kccot_pairwise_cost3_f32(gi["real"].ptr, gi["fake"].ptr, B, K, SC, *(gi[k].ptr for k in FEATS), T, J,
                                                L.COST_GRAM_SUMS_ONLY, c3.ptr, gw.ptr, ws, None)
            torch.cuda.synchronize()
            assert rc == 0, L.lib.kccot_last_error()
            assert all(g.verify() is None for g in [gw, c3] + list(gi.values()))
            assert bool(ag.unwritten(c3.view(F32, (3, B, B))).all()), "GRAM_SUMS_ONLY wrote C3"
            span = gw.payload()[off.value:off.value + 8 * nd.value].clone()
            got = guarded_call(L, "kccot_pairwise_cost3_f32", spec(L.COST_FROM_GRAM_SUMS), ins, {"C3": ((3, B, B), F32)}, ws,
                               ws_keep=(off.value, 8 * nd.value, span))["C3"]
    return (got,) + expect(T, J, ("xy", "xx", "yy"), slice(0, B), B)


def _rows(L, T, J, B, rb, rc, gram):
    ins = _cost3_ins(T, J, B)
    if gram:
        assert L.lib.kccot_pairwise_cost3_rows_gram_supported(rc, B, K) == 1
        ins["norms"] = torch.zeros(B, 3, dtype=F64, device=DEV)         # x.x, e.e, x.e of zero videos
        ws = ws_query(L, "kccot_pairwise_cost3_rows_gram_workspace_bytes", rc, B, K)
        sym, mid = "kccot_pairwise_cost3_rows_gram_f32", ["@norms"]
    else:
        ws = ws_query(L, "kccot_pairwise_cost3_rows_workspace_bytes", rc, B, K)
        sym, mid = "kccot_pairwise_cost3_rows_f32", []
    spec = ["@real", "@fake", B, K, SC, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J, rb, rc] + mid + ["@C3_rows", "@ws",
                                                                                                         "@ws_bytes", None]
    got = guarded_call(L, sym, spec, ins, {"C3_rows": ((3, rc, B), F32)}, ws)["C3_rows"]
    return (got,) + expect(T, J, ("xy", "xx", "yy"), slice(rb, rb + rc), B)


def _in_place(L, T, J, call, shape, inputs):
    """An entry point whose output is input AND output, on a zero block: (result, guarded inputs verified)."""
    gC = ag.guarded_input("C", _zeros(*shape))
    gi = {k: ag.guarded_input(k, v) for k, v in inputs.items()}
    snap = {k: g.payload().clone() for k, g in gi.items()}
    rc = call(gC, gi)
    torch.cuda.synchronize()
    assert rc == 0, L.lib.kccot_last_error()
    bad = [m for m in (g.verify() for g in [gC] + list(gi.values())) if m]
    assert not bad, "guard zone damaged: " + "; ".join(bad)
    for k, g in gi.items():
        assert torch.equal(g.payload(), snap[k]), "the call wrote its input %s" % k
    return gC.view(F32, shape).clone()


def _bicausal(L, T, J, B):
    got = _in_place(L, T, J, lambda gC, gi: L.lib.kccot_pairwise_cost3_f32(
        None, None, B, 0, SC, *(gi[k].ptr for k in FEATS), T, J, L.COST_BICAUSAL_TERM_ONLY, gC.ptr, None, 0, None),
        (3, B, B), {k: dev(T, J, k, B) for k in FEATS})
    return (got,) + expect(T, J, ("bxy", "xx", "yy"), slice(0, B), B)


FWD = {
    "pair_direct": lambda L, T, J: _pair(L, T, J, 17, 33, L.COST_FORCE_DIRECT),
    "pair_direct_h2": lambda L, T, J: _pair(L, T, J, 17, 33, L.COST_FORCE_DIRECT, two=True),
    "pair_same_direct": lambda L, T, J: _pair(L, T, J, 33, 33, L.COST_FORCE_DIRECT, same=True),
    "pair_mfma": lambda L, T, J: _pair(L, T, J, 17, 33, L.COST_FORCE_MFMA),
    "pair_mfma_h2": lambda L, T, J: _pair(L, T, J, 17, 33, L.COST_FORCE_MFMA, two=True),
    "pair_same_mfma": lambda L, T, J: _pair(L, T, J, 33, 33, L.COST_FORCE_MFMA, same=True),
    "cost3_b64": lambda L, T, J: _cost3(L, T, J, 64, {}),
    "cost3_b40": lambda L, T, J: _cost3(L, T, J, 40, {}),
    "cost3_b24": lambda L, T, J: _cost3(L, T, J, 24, {}),
    "cost3_b64_gram_f32": lambda L, T, J: _cost3(L, T, J, 64, dict(gram_f32=1)),
    "cost3_b64_split": lambda L, T, J: _cost3(L, T, J, 64, {}, split=True),
    "cost3_b192": lambda L, T, J: _cost3(L, T, J, 192, {}),
    "cost3_b128_tiles128": lambda L, T, J: _cost3(L, T, J, 128, dict(cost_tile256=0)),
    "cost3_b128": lambda L, T, J: _cost3(L, T, J, 128, {}),
    "cost3_b256": lambda L, T, J: _cost3(L, T, J, 256, {}),
    "rows_b65": lambda L, T, J: _rows(L, T, J, 65, 3, 61, False),
    "rows_gram_32_128": lambda L, T, J: _rows(L, T, J, 128, 32, 32, True),
    "rows_gram_64_256": lambda L, T, J: _rows(L, T, J, 256, 128, 64, True),
    "bicausal_b17": lambda L, T, J: _bicausal(L, T, J, 17),
    "bicausal_b64": lambda L, T, J: _bicausal(L, T, J, 64),
}


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("host", list(FWD))
def test_causal_term_on_every_host(L, host, shape):
    T, J = shape
    got, w64, w32, S = FWD[host](L, T, J)
    check(host, T, J, got, w64, w32, S)
    if T == 1:
        assert ag.same_bits(got.cpu(), torch.zeros(got.shape) * torch.tensor(SC)), "%s: T = 1 must give the bits of sc 0" % host


@pytest.mark.parametrize("shape", [(258, 1), (2, 300), (65, 16)], ids=SHAPE_ID)
def test_causal_add_past_one_chunk(L, shape):
    """KCCOT_COST_CAUSAL_ADD at the shapes of the table that test_gpu_mixed_flag_bounds.py lacks."""
    T, J = shape
    Bx, By = 17, 33
    got = _in_place(L, T, J, lambda gC, gi: L.lib.kccot_pairwise_cost_f32(
        None, None, Bx, By, 0, SC, gi["h"].ptr, gi["M"].ptr, None, None, T, J, L.COST_CAUSAL_ADD, gC.ptr, None, 0, None),
        (Bx, By), {"h": dev(T, J, "h_fake", Bx), "M": dev(T, J, "m_real", By)})
    w64, w32, S = expect(T, J, ("xy",), slice(0, Bx), By)
    check("causal_add", T, J, got, w64[0], w32[0], S[0])


# ---------------------------------------------------------------- backward
def _abs_terms(h, M):
    """sc (sum_k h |dM|  +  sum_k |h| (M[t+1] + M[t])): its gradient w.r.t. h is the S of dh, w.r.t. M the S of dM."""
    n, m = h.shape[0], M.shape[0]
    hf = h[:, :-1].reshape(n, -1)
    dM = (M[:, 1:] - M[:, :-1]).detach().abs().reshape(m, -1)
    return SC * (hf @ dM.t() + hf.detach().abs() @ (M[:, 1:] + M[:, :-1]).reshape(m, -1).t())


@functools.lru_cache(maxsize=None)
def grads(T, J, terms, seed, gscale=1.0):
    """terms: ((h name, rows, M name, rows), ...), one per matrix of dC (seeded randn, times gscale).
    Returns (dC fp32 [len(terms), rows, cols] list, name -> (fp64 autograd, fp32 autograd, S))."""
    g = torch.Generator().manual_seed(seed)
    dC = [torch.randn(nh, nm, generator=g) for _, nh, _, nm in terms]
    sizes = {}
    for hk, nh, mk, nm in terms:
        sizes[hk], sizes[mk] = nh, nm
    names = sorted(sizes)
    res = {}
    for dt in (F64, F32):
        f = {k: feats(T, J)[k][:sizes[k]].to(dt).requires_grad_(True) for k in names}
        tot = sum((ot.causal_term(f[hk], f[mk], SC) * (d.double() * gscale).to(dt)).sum() for (hk, _, mk, _), d in zip(terms, dC))
        res[dt] = dict(zip(names, torch.autograd.grad(tot, [f[k] for k in names])))
    f = {k: feats(T, J)[k][:sizes[k]].double().requires_grad_(True) for k in names}
    tot = sum((_abs_terms(f[hk], f[mk]) * (d.double() * gscale).abs()).sum() for (hk, _, mk, _), d in zip(terms, dC))
    S = dict(zip(names, torch.autograd.grad(tot, [f[k] for k in names])))
    return dC, {k: (res[F64][k], res[F32][k], S[k]) for k in names}


def _loss3_terms(B):
    return tuple((h, B, m, B) for h, m in (PAIRS["xy"], PAIRS["xx"], PAIRS["yy"]))


def _cost3_bwd(L, label, T, J, B, opts, rows=None, gscale=None):
    dC, ref = grads(T, J, _loss3_terms(B), 7 * B + T * J, gscale or 1.0)
    rb, rc = rows or (0, B)
    ins = {"g3": torch.stack(dC).to(DEV), **_cost3_ins(T, J, B)}
    outs = {"dfake": ((rc, K), F32), **{"d" + k: ((rc, T, J), F32) for k in FEATS}}
    mid = ["@real", "@fake", B, K, SC, "@h_fake", "@h_real", "@m_real", "@m_fake", T, J]
    tail = ["@dfake", "@dh_fake", "@dh_real", "@dm_real", "@dm_fake", "@ws", "@ws_bytes", None]
    ws = ws_query(L, "kccot_pairwise_cost3_bwd_workspace_bytes", B, K)
    with L.options(**opts):
        if rows:
            res = guarded_call(L, "kccot_pairwise_cost3_bwd_rows_f32", ["@g3"] + mid + [rb, rc] + tail, ins, outs, ws)
        elif gscale is not None:
            ins["gscale"] = torch.tensor([gscale], device=DEV)
            res = guarded_call(L, "kccot_pairwise_cost3_bwd_scaled_f32", ["@g3", "@gscale"] + mid + tail, ins, outs, ws)
        else:
            res = guarded_call(L, "kccot_pairwise_cost3_bwd_f32", ["@g3"] + mid + tail, ins, outs, ws)
    assert bool((res["dfake"] == 0).all()), "%s: dfake of zero videos must be exactly zero" % label
    check_case(label, T, J, {"d" + k: (res["d" + k],) + tuple(x[rb:rb + rc] for x in ref[k]) for k in FEATS})


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_ID)
@pytest.mark.parametrize("one_launch", [1, 0])
def test_feature_gradients_b64_both_forms(L, one_launch, shape):
    _cost3_bwd(L, "bwd_b64_%s" % ("one" if one_launch else "two"), shape[0], shape[1], 64, dict(apply_one_launch=one_launch))


@pytest.mark.parametrize("shape", PAST, ids=SHAPE_ID)
@pytest.mark.parametrize("B,form", [(40, "one"), (40, "two"), (8, "one"), (8, "two"), (128, "chunks"), (192, "chunks")])
def test_feature_gradients_other_batches(L, B, form, shape):
    """B = 40, 8: the one-launch and two-launch forms; B = 128, 192: two and three batch chunks of coeffs_and_causal_grads."""
    _cost3_bwd(L, "bwd_b%d_%s" % (B, form), shape[0], shape[1], B, dict(apply_one_launch=0 if form == "two" else 1))


@pytest.mark.parametrize("shape", PAST, ids=SHAPE_ID)
def test_feature_gradients_scaled(L, shape):
    _cost3_bwd(L, "scaled_b64", shape[0], shape[1], 64, {}, gscale=-1.75)


@pytest.mark.parametrize("shape", PAST, ids=SHAPE_ID)
@pytest.mark.parametrize("B,rows", [(65, (3, 60)), (128, (32, 64))])
def test_feature_gradients_of_a_row_block(L, B, rows, shape):
    _cost3_bwd(L, "rows_b%d" % B, shape[0], shape[1], B, {}, rows=rows)


@pytest.mark.parametrize("shape", PAST, ids=SHAPE_ID)
@pytest.mark.parametrize("Bx,By,same", [(17, 33, False), (33, 33, True)])
def test_feature_gradients_of_one_matrix(L, Bx, By, same, shape):
    T, J = shape
    hk = "h_real" if same else "h_fake"
    dC, ref = grads(T, J, ((hk, Bx, "m_real", By),), 11 * Bx + T * J)
    ins = {"g": dC[0].to(DEV), "x": _zeros(Bx, K), "h": dev(T, J, hk, Bx), "M": dev(T, J, "m_real", By)}
    outs = {"dx": ((Bx, K), F32), "dh": ((Bx, T, J), F32), "dM": ((By, T, J), F32)}
    if not same:
        ins["y"], outs["dy"] = _zeros(By, K), ((By, K), F32)
    spec = ["@g", "@x", "@x" if same else "@y", Bx, By, K, SC, "@h", "@M", T, J, L.COST_SAME if same else 0, "@dx",
            None if same else "@dy", "@dh", "@dM", "@ws", "@ws_bytes", None]
    res = guarded_call(L, "kccot_pairwise_cost_bwd_f32", spec, ins, outs,
                       ws_query(L, "kccot_pairwise_cost_bwd_workspace_bytes", Bx, By))
    label = "pair_same" if same else "pair"
    assert all(bool((res[k] == 0).all()) for k in outs if k in ("dx", "dy")), "%s: zero videos, zero video gradients" % label
    check_case(label, T, J, {"dh": (res["dh"],) + ref[hk], "dM": (res["dM"],) + ref["m_real"]})


# ---------------------------------------------------------------- the two losses past one chunk
def test_bicausal_loss_past_one_chunk(G):
    """The two-term jobs of dh_real / dm_fake and bicausal_cost_add inside the loss: random videos, (T, J) = (34, 8); oracle
    and tolerances of test_gpu_bicausal_loss.py::test_bicausal_loss_on_random_ragged_shapes (near regime)."""
    inp = BL._rand_inputs(16, 260, 34, 8, seed=1)
    BL._check_against_oracle(G, inp, BL.WRT, cases.SC, 4 * 2.5e-5, loss_abs=2e-6, tag="past one chunk")


def test_mixed_loss_past_one_chunk(G):
    """The four-problem stack: oracle and tolerances of test_gpu_mixed_loss.py::test_mixed_loss_on_random_ragged_shapes."""
    inp = ML._rand_inputs(16, 260, 34, 8, seed=1)
    ML._check_mix(ML._run(G, inp), ML._ref(inp), gtol=4 * 2.5e-5, loss_abs=2e-6)
